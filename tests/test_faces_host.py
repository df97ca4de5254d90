"""CPU: per-face identification and the face-to-person match (prpe.faces, csrc/roi.hip) as far as
the host goes -- the ABI table and the refusals, plain-torch restatements of the three rules
(``roi_select_ref``, ``roi_resize_ref``, ``face_person_match_ref``, which tests/test_gpu_faces.py
holds the kernels to), a second statement of the match written apart from the first, and the
host helpers of ``FaceCrops`` / ``PersonRecognition``."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import test_topdown_host as T
from prpe import _lib

NAN, INF = float("nan"), float("inf")
_f = T._f


# ---------------------------------------------------------------------------------- roi_select
def roi_window_ref(x1, y1, x2, y2, pad, out_hw):
    """(x0, y0, w, h) of include/prpe.h's window for an out_h x out_w output: every step one fp32
    operation on 0-dim float32 tensors; the aspect is the fp32 quotient out_w / out_h."""
    x1, y1, x2, y2, pad = (_f(v) for v in (x1, y1, x2, y2, pad))
    a = _f(out_hw[1]) / _f(out_hw[0])
    cx, cy = (x1 + x2) * 0.5, (y1 + y2) * 0.5
    w, h = x2 - x1, y2 - y1
    if bool(w > a * h):
        h = w / a
    else:
        w = h * a
    w, h = w * pad, h * pad
    return cx - 0.5 * w, cy - 0.5 * h, w, h


def roi_select_ref(dets, counts, out_hw, score_thr=0.25, max_per_frame=8, min_size=4.0, box_scale=(1.0, 1.0),
                   pad=1.25, max_crops=8):
    """prpe_roi_select on the host: (crop_meta [max_crops, 8] float32, n_crops, status)."""
    dets = dets.float().cpu()
    sx, sy = _f(box_scale[0]), _f(box_scale[1])
    thr, mins = _f(score_thr), _f(min_size)
    rows, status = [], 0
    for b, c in enumerate(int(v) for v in counts):
        if c < 0:
            status |= 1
            continue
        pre = 0
        while pre < min(c, dets.shape[1], max_per_frame) and bool(dets[b, pre, 4] >= thr):
            pre += 1
        for r in range(pre):
            x1, y1, x2, y2 = dets[b, r, 0] * sx, dets[b, r, 1] * sy, dets[b, r, 2] * sx, dets[b, r, 3] * sy
            if not all(bool(torch.isfinite(v)) for v in (x1, y1, x2, y2)):
                continue
            if not bool(x2 - x1 >= mins) or not bool(y2 - y1 >= mins):
                continue
            win = roi_window_ref(x1, y1, x2, y2, pad, out_hw)
            if not all(bool(torch.isfinite(v)) for v in win):
                continue
            rows.append((b, r, *win, dets[b, r, 4]))
    if len(rows) > max_crops:
        status |= 2
        rows = rows[:max_crops]
    meta = torch.zeros(max_crops, 8, dtype=torch.float32)
    ints = meta.view(torch.int32)
    ints[:, 0] = -1
    for s, (b, r, x0, y0, w, h, score) in enumerate(rows):
        ints[s, 0], ints[s, 1] = b, r
        meta[s, 2], meta[s, 3], meta[s, 4], meta[s, 5], meta[s, 6] = x0, y0, w, h, score
    return meta, len(rows), status


@pytest.mark.parametrize("name", sorted(T.select_edge_cases()))
def test_roi_select_ref_at_256x192_is_the_crop_list_rule(name):
    """At the ViTPose size the restatement has ``select_ref``'s bits on every edge case of
    tests/test_topdown_host.py (which holds ``select_ref`` to a numpy statement of the rule)."""
    dets, counts, kw, want_n, want_status, _ = T.select_edge_cases()[name]
    meta, n, status = roi_select_ref(dets, counts, (256, 192), **kw)
    ref, n_ref, st_ref = T.select_ref(dets, counts, **kw)
    assert (n, status) == (n_ref, st_ref) == (want_n, want_status)
    assert torch.equal(meta.view(torch.int32), ref.view(torch.int32))


def test_roi_window_on_hand_cases():
    # a square output: a square box stays (w == a h takes the else branch), pad 1.25 about (30, 40)
    assert [float(v) for v in roi_window_ref(20, 30, 40, 50, 1.25, (112, 112))] == [17.5, 27.5, 25.0, 25.0]
    # tall box 10 x 40 at 112 x 112: w grows to 40; wide box 40 x 10: h grows to 40
    assert [float(v) for v in roi_window_ref(0, 0, 10, 40, 1.0, (112, 112))] == [-15.0, 0.0, 40.0, 40.0]
    assert [float(v) for v in roi_window_ref(0, 0, 40, 10, 1.0, (112, 112))] == [0.0, -15.0, 40.0, 40.0]
    # 8 x 12 (h x w): a = 1.5; 30 x 20 is exactly 1.5 (else branch), 20 x 20 grows to 30 wide
    assert [float(v) for v in roi_window_ref(0, 0, 30, 20, 1.0, (8, 12))] == [0.0, 0.0, 30.0, 20.0]
    assert [float(v) for v in roi_window_ref(0, 0, 20, 20, 1.0, (8, 12))] == [-5.0, 0.0, 30.0, 20.0]
    # an aspect that is not a dyadic number rounds once: 112 / 96 in fp32
    x0, y0, w, h = roi_window_ref(0, 0, 10, 96, 1.0, (96, 112))
    assert float(w) == float(_f(96.0) * (_f(112.0) / _f(96.0))) and float(h) == 96.0


# ---------------------------------------------------------------------------------- roi_resize
def roi_resize_ref(frames64, f, win, out_hw, round_grid=False):
    """The yardstick: F.affine_grid + F.grid_sample(bilinear, zeros, align_corners=False) in
    float64 on the window ``win`` = (x0, y0, w, h) of frame ``f`` -> [3, out_h, out_w].
    ``round_grid``: the same with the sampling grid rounded to fp32 (the yardstick's own fp32
    noise: the tests allow the kernel 4 x that)."""
    H, W = frames64.shape[2:]
    x0, y0, w, h = (float(v) for v in win)
    theta = torch.tensor([[[w / W, 0.0, (2 * x0 + w) / W - 1.0], [0.0, h / H, (2 * y0 + h) / H - 1.0]]],
                         dtype=torch.float64)
    grid = F.affine_grid(theta, (1, 3, out_hw[0], out_hw[1]), align_corners=False)
    if round_grid:
        grid = grid.float().double()
    return F.grid_sample(frames64[f:f + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]


def test_roi_resize_ref_identity_and_shift():
    g = torch.Generator().manual_seed(3)
    fr = torch.rand(2, 3, 6, 9, generator=g, dtype=torch.float64)
    assert torch.allclose(roi_resize_ref(fr, 1, (0.0, 0.0, 9.0, 6.0), (6, 9)), fr[1], atol=1e-14, rtol=0)
    # a window one pixel to the right: column j samples column j + 1, the last one is outside (0)
    y = roi_resize_ref(fr, 0, (1.0, 0.0, 9.0, 6.0), (6, 9))
    assert torch.allclose(y[:, :, :8], fr[0, :, :, 1:], atol=1e-14, rtol=0) and float(y[:, :, 8].abs().max()) == 0.0
    # 1 x 1 output of the whole frame: the centre, the mean of the four middle pixels (9 is odd: two)
    y = roi_resize_ref(fr, 0, (0.0, 0.0, 9.0, 6.0), (1, 1))
    assert torch.allclose(y[:, 0, 0], (fr[0, :, 2, 4] + fr[0, :, 3, 4]) / 2, atol=1e-14, rtol=0)


# ---------------------------------------------------------------------------------- the match
def face_person_match_ref(meta_p, n_p, kpts, meta_f, n_f, ident, score, B, kp_thr=0.3, head_kpts=5):
    """prpe_face_person_match on the host, a loop per pair in fp32 (0-dim float32 tensors: every
    operation rounds once): (face_slot [P] int32, ident [P] int64, score [P] float32, status [B]
    int32)."""
    P = meta_p.shape[0]
    pf, pi = meta_p.float(), meta_p.view(torch.int32)
    ff, fi = meta_f.float(), meta_f.view(torch.int32)
    n_p, n_f = max(0, min(int(n_p), P)), max(0, min(int(n_f), meta_f.shape[0]))
    thr = _f(kp_thr)
    face_slot = torch.full((P,), -1, dtype=torch.int32)
    out_ident = torch.full((P,), -1, dtype=torch.int64)
    out_score = torch.full((P,), -INF, dtype=torch.float32)
    status = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        ps = [s for s in range(n_p) if int(pi[s, 0]) == b]
        fs = [s for s in range(n_f) if int(fi[s, 0]) == b]
        if len(ps) > 32 or len(fs) > 32:
            status[b] = 1
            continue
        heads = []
        for s in ps:
            x0, y0, w, h = pf[s, 2], pf[s, 3], pf[s, 4], pf[s, 5]
            sx, sy, cnt = _f(0.0), _f(0.0), 0
            for k in range(head_kpts):
                if bool(kpts[s, k, 2] >= thr):
                    sx, sy, cnt = sx + kpts[s, k, 0], sy + kpts[s, k, 1], cnt + 1
            heads.append((sx / _f(cnt), sy / _f(cnt)) if cnt else (x0 + 0.5 * w, y0 + 0.25 * h))
        cost = {}
        for i, s in enumerate(ps):
            x0, y0, x1, y1 = pf[s, 2], pf[s, 3], pf[s, 2] + pf[s, 4], pf[s, 3] + pf[s, 5]
            for j, t in enumerate(fs):
                cx, cy = ff[t, 2] + 0.5 * ff[t, 4], ff[t, 3] + 0.5 * ff[t, 5]
                dx, dy = heads[i][0] - cx, heads[i][1] - cy
                c = dx * dx + dy * dy
                if bool(cx >= x0) and bool(cx <= x1) and bool(cy >= y0) and bool(cy <= y1) and bool(torch.isfinite(c)):
                    cost[(i, j)] = float(c)
        free_p, free_f = set(range(len(ps))), set(range(len(fs)))
        while True:                                   # the least eligible pair left, ties: person, then face
            best = None
            for (i, j), c in cost.items():
                if i in free_p and j in free_f and (best is None or (c, i, j) < best):
                    best = (c, i, j)
            if best is None:
                break
            _, i, j = best
            free_p.discard(i)
            free_f.discard(j)
            face_slot[ps[i]], out_ident[ps[i]], out_score[ps[i]] = fs[j], ident[fs[j]], score[fs[j]]
    return face_slot, out_ident, out_score, status


def match_plain(meta_p, n_p, kpts, meta_f, n_f, ident, score, B, kp_thr=0.3, head_kpts=5):
    """include/prpe.h's match once more, on numpy float32 scalars, as one sorted walk over the
    eligible pairs (a greedy choice on fixed costs takes the pairs in sorted order and skips those
    with a matched end): written apart from ``face_person_match_ref`` and sharing no code with it."""
    f = np.float32
    mp, mf = meta_p.numpy(), meta_f.numpy()
    fp, ffr = mp.view(np.int32)[:, 0], mf.view(np.int32)[:, 0]
    kp = kpts.numpy().astype(np.float32)
    P = mp.shape[0]
    n_p, n_f = min(max(int(n_p), 0), P), min(max(int(n_f), 0), mf.shape[0])
    face = np.full(P, -1, np.int32)
    oid = np.full(P, -1, np.int64)
    osc = np.full(P, -np.inf, np.float32)
    status = np.zeros(B, np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            persons = np.nonzero(fp[:n_p] == b)[0]
            faces = np.nonzero(ffr[:n_f] == b)[0]
            if persons.size > 32 or faces.size > 32:
                status[b] = 1
                continue
            pairs = []
            for s in persons:
                x0, y0, w, h = (f(v) for v in mp[s, 2:6])
                good = [k for k in range(head_kpts) if kp[s, k, 2] >= f(kp_thr)]
                if good:
                    hx = hy = f(0)
                    for k in good:
                        hx, hy = f(hx + kp[s, k, 0]), f(hy + kp[s, k, 1])
                    hx, hy = f(hx / f(len(good))), f(hy / f(len(good)))
                else:
                    hx, hy = f(x0 + f(f(0.5) * w)), f(y0 + f(f(0.25) * h))
                for t in faces:
                    cx = f(mf[t, 2] + f(f(0.5) * mf[t, 4]))
                    cy = f(mf[t, 3] + f(f(0.5) * mf[t, 5]))
                    if not (x0 <= cx <= f(x0 + w) and y0 <= cy <= f(y0 + h)):
                        continue
                    dx, dy = f(hx - cx), f(hy - cy)
                    c = f(f(dx * dx) + f(dy * dy))
                    if math.isfinite(c):
                        pairs.append((float(c), int(s), int(t)))
            used_p, used_f = set(), set()
            for c, s, t in sorted(pairs):
                if s not in used_p and t not in used_f:
                    used_p.add(s)
                    used_f.add(t)
                    face[s], oid[s], osc[s] = t, int(ident[t]), f(score[t])
    return face, oid, osc, status


K = 7                                                 # keypoints per person in the cases (5 of the head)


def _lists(frames, max_p=None, max_f=None, stale=True):
    """frames: per frame (persons, faces); a person = ((x0, y0, w, h), [(x, y, score)] * <= K), a
    face = ((x0, y0, w, h), ident, score). -> (meta_p, n_p, kpts, meta_f, n_f, ident, score, B)
    as the stages lay them out; rows behind n_p / n_f are stale rows of a longer earlier list
    (frame indices that look valid, finite windows) when ``stale``."""
    persons = [(b, *p) for b, (ps, _) in enumerate(frames) for p in ps]
    faces = [(b, *q) for b, (_, fs) in enumerate(frames) for q in fs]
    P = max_p or len(persons) + 3
    Fn = max_f or len(faces) + 2
    mp, mf = torch.zeros(P, 8), torch.zeros(Fn, 8)
    mp.view(torch.int32)[:, 0] = -1
    mf.view(torch.int32)[:, 0] = -1
    kp = torch.zeros(P, K, 3)
    ident = torch.full((Fn,), -1, dtype=torch.int64)
    score = torch.full((Fn,), -INF)
    for s, (b, win, pts) in enumerate(persons):
        mp.view(torch.int32)[s, 0], mp.view(torch.int32)[s, 1] = b, s
        mp[s, 2:6] = torch.tensor(win, dtype=torch.float32)
        mp[s, 6] = 0.9
        for k, pt in enumerate(pts):
            kp[s, k] = torch.tensor(pt, dtype=torch.float32)
    for s, (b, win, idn, sc) in enumerate(faces):
        mf.view(torch.int32)[s, 0], mf.view(torch.int32)[s, 1] = b, s
        mf[s, 2:6] = torch.tensor(win, dtype=torch.float32)
        mf[s, 6] = 0.8
        ident[s], score[s] = idn, sc
    if stale:
        for s in range(len(persons), P):              # what a longer list of an earlier call left
            mp.view(torch.int32)[s, 0] = s % len(frames)
            mp[s, 2:6] = torch.tensor([0.0, 0.0, 200.0, 200.0])
            kp[s, :, :] = torch.tensor([50.0, 50.0, 0.9])
        for s in range(len(faces), Fn):
            mf.view(torch.int32)[s, 0] = s % len(frames)
            mf[s, 2:6] = torch.tensor([40.0, 40.0, 20.0, 20.0])
            ident[s], score[s] = 999, 0.99
    return mp, len(persons), kp, mf, len(faces), ident, score, len(frames)


def _person(win, head, others=0.9):
    """A person whose 5 head keypoints all sit at ``head`` with score 0.9 (two body points elsewhere)."""
    return (win, [(head[0], head[1], others)] * 5 + [(win[0], win[1], 0.9)] * 2)


def match_edge_cases():
    """name -> (arguments of the match, expected face_slot per person slot below n_p, expected
    status). The expectations are literals worked out by hand from include/prpe.h."""
    cases = {}
    big = (0.0, 0.0, 100.0, 100.0)
    frames = [
        ([], [((10.0, 10.0, 20.0, 20.0), 7, 0.5)]),                                   # 0: a face, nobody
        ([_person(big, (50.0, 20.0))], []),                                           # 1: a person, no face
        ([], []),                                                                     # 2: neither
        # 3: one face (centre 50, 30) inside two windows: head (52, 30) is nearer than (40, 30)
        ([_person(big, (40.0, 30.0)), _person((20.0, 0.0, 80.0, 90.0), (52.0, 30.0))],
         [((40.0, 20.0, 20.0, 20.0), 11, 0.7)]),
        ([], []),                                                                     # 4: empty again
        # 5: two faces (centres 40, 50 and 60, 50) at cost 100 each from the head (50, 50): the lower slot
        ([_person(big, (50.0, 50.0))], [((30.0, 40.0, 20.0, 20.0), 21, 0.6), ((50.0, 40.0, 20.0, 20.0), 22, 0.65)]),
        # 6: two persons (heads 40, 50 and 60, 50) at cost 100 each from one face (50, 50): the lower slot
        ([_person(big, (40.0, 50.0)), _person(big, (60.0, 50.0))], [((45.0, 45.0, 10.0, 10.0), 31, 0.75)]),
        # 7: the face centre (30, 20) exactly on the window's right edge x0 + w = 30 (eligible), and
        # every head keypoint below kp_thr: the fallback (x0 + w / 2, y0 + h / 4) = (20, 15)
        ([((10.0, 5.0, 20.0, 40.0), [(99.0, 99.0, 0.29)] * 5 + [(15.0, 40.0, 0.9)] * 2)],
         [((25.0, 15.0, 10.0, 10.0), 41, 0.8)]),
        # 8: person 0 has exactly one head keypoint at kp_thr (>= keeps it), the others below; person
        # 1 has a NaN head keypoint above the threshold: its cost is NaN, it never matches, although
        # the second face lies in its window
        ([(big, [(30.0, 30.0, 0.3)] + [(90.0, 90.0, 0.1)] * 4 + [(0.0, 0.0, 0.9)] * 2),
          (big, [(NAN, 60.0, 0.9)] + [(60.0, 60.0, 0.9)] * 4 + [(0.0, 0.0, 0.9)] * 2)],
         [((25.0, 25.0, 10.0, 10.0), 51, 0.85), ((55.0, 55.0, 10.0, 10.0), 52, 0.86)]),
        # 9: the face centre one fp32 outside the window: nobody
        ([_person((10.0, 10.0, 20.0, 20.0), (20.0, 20.0))],
         [((float(torch.nextafter(_f(30.0), _f(INF))) - 5.0, 15.0, 10.0, 10.0), 61, 0.9)]),
    ]
    # person slots: f1 -> 0; f3 -> 1, 2; f5 -> 3; f6 -> 4, 5; f7 -> 6; f8 -> 7, 8; f9 -> 9
    # face slots:   f0 -> 0; f3 -> 1; f5 -> 2, 3; f6 -> 4; f7 -> 5; f8 -> 6, 7; f9 -> 8
    cases["edges"] = (_lists(frames), [-1, -1, 1, 2, 4, -1, 5, 6, -1, -1], [0] * 10)
    assert float(_f(25.0) + _f(0.5) * _f(10.0)) == 30.0

    # 32 x 32 in one frame (every face inside every window), 33 persons in the next (status 1, no
    # match), then an ordinary frame, then 33 faces (status 1)
    g = torch.Generator().manual_seed(21)
    heads = (torch.rand(32, 2, generator=g) * 80 + 10).tolist()
    centres = (torch.rand(32, 2, generator=g) * 80 + 10).tolist()
    full = ([_person(big, tuple(h)) for h in heads],
            [((c[0] - 4.0, c[1] - 4.0, 8.0, 8.0), 100 + j, 0.5 + j / 100) for j, c in enumerate(centres)])
    over_p = ([_person(big, (50.0, 50.0))] * 33, [((46.0, 46.0, 8.0, 8.0), 200, 0.9), ((10.0, 10.0, 8.0, 8.0), 201, 0.8)])
    plain = ([_person(big, (50.0, 50.0))], [((46.0, 46.0, 8.0, 8.0), 300, 0.95)])
    over_f = ([_person(big, (50.0, 50.0))] * 2, [((46.0, 46.0, 8.0, 8.0), 400 + j, 0.7) for j in range(33)])
    args = _lists([full, over_p, plain, over_f])
    cases["full"] = (args, None, [0, 1, 0, 1])        # the 32 x 32 assignment: the two statements agree
    # nothing at all: n_p = n_f = 0 with stale rows behind
    cases["empty"] = (_lists([([], []), ([], [])], max_p=4, max_f=3), [], [0, 0])
    return cases


@pytest.mark.parametrize("name", sorted(match_edge_cases()))
def test_match_ref_equals_the_plain_statement_and_the_literals(name):
    args, want_face, want_status = match_edge_cases()[name]
    face, ident, score, status = face_person_match_ref(*args)
    face2, ident2, score2, status2 = match_plain(*args)
    assert np.array_equal(face.numpy(), face2) and np.array_equal(ident.numpy(), ident2)
    assert np.array_equal(score.numpy().view(np.int32), score2.view(np.int32))
    assert status.tolist() == status2.tolist() == want_status
    n_p = args[1]
    if want_face is not None:
        assert face[:n_p].tolist() == want_face
    assert bool((face[n_p:] == -1).all()) and bool((ident[n_p:] == -1).all()) and bool((score[n_p:] == -INF).all())
    f_ident, f_score = args[5], args[6]
    for s in range(n_p):                              # ident and score are the matched face's
        t = int(face[s])
        assert (int(ident[s]), float(score[s])) == ((int(f_ident[t]), float(f_score[t])) if t >= 0 else (-1, -INF))
    hit = face[face >= 0].tolist()
    assert len(hit) == len(set(hit))                  # one-to-one


def test_match_full_frame_is_a_complete_assignment():
    args, _, _ = match_edge_cases()["full"]
    face, _, _, status = face_person_match_ref(*args)
    assert sorted(face[:32].tolist()) == list(range(32))                # 32 x 32, all eligible: everybody matched
    assert bool((face[32:65] == -1).all()) and int(face[65]) == 34      # 33 persons: none; the plain frame: its face
    assert face[66:68].tolist() == [-1, -1] and status.tolist() == [0, 1, 0, 1]


# ---------------------------------------------------------------------------------- ABI
ENTRY_POINTS = (("prpe_roi_select", 19), ("prpe_roi_resize", 7), ("prpe_roi_resize_u8", 10),
                ("prpe_face_person_match", 18))


def test_abi_table_has_the_roi_entry_points_and_the_abi_is_still_12():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert _lib.ABI_VERSION == 12
    assert int(re.search(r"#define PRPE_ABI_VERSION (\d+)", header).group(1)) == 12
    for name, nargs in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/prpe.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().prpe_abi_version() == 12


def test_library_rejects_bad_roi_arguments_before_launch():
    L = _lib.lib()
    p = 0x1000

    def select(dets=p, pad=1.25, out_h=112, out_w=112, max_crops=4, sx=1.0):
        return L.prpe_roi_select(dets, p, 1, 1, 0.25, 8, 4.0, sx, 1.0, 64, 64, pad, out_h, out_w, max_crops, p, p, p,
                                 None)
    assert select(dets=None) == -22
    assert select(max_crops=0) == -22
    assert select(pad=0.0) == -22 and select(pad=NAN) == -22 and select(sx=NAN) == -22
    for bad in (0, -1, 4097):
        assert select(out_h=bad) == -22 and select(out_w=bad) == -22
    fr = _lib.View(p, 1, 8, 8, 3, 192, 24, 3, 1)
    fr4 = _lib.View(p, 1, 8, 8, 4, 256, 32, 4, 1)
    a3 = (C.c_float * 3)(1.0, 1.0, 1.0)

    def y(ptr=p, n=2, h=12, w=12, c=4, sn=12 * 16 * 4, sh=16 * 4, sw=4, sc=1):
        return _lib.View(ptr, n, h, w, c, sn, sh, sw, sc)

    def both(frames=fr, meta=p, n_crops=p, max_crops=2, yv=None):
        yv = y() if yv is None else yv
        r1 = L.prpe_roi_resize(C.byref(frames), meta, n_crops, max_crops, C.byref(yv), None, None)
        r2 = L.prpe_roi_resize_u8(C.byref(frames), meta, n_crops, max_crops, a3, a3, 0, C.byref(yv), None, None)
        assert r1 == r2
        return r1
    assert both(frames=fr4) == -22                    # 4-channel frames
    assert both(meta=None) == -22 and both(n_crops=None) == -22
    assert both(max_crops=0) == -22 and both(max_crops=3) == -22       # no slot; not the view's n
    assert both(yv=y(ptr=None)) == -22
    assert both(yv=y(sc=2)) == -22                    # channels not contiguous
    assert both(yv=y(ptr=p + 4)) == -22               # not 16-byte aligned
    assert both(yv=y(sw=6)) == -22 and both(yv=y(sh=66)) == -22 and both(yv=y(sn=12 * 16 * 4 + 2)) == -22
    assert both(yv=y(c=3)) == -22
    assert both(yv=y(h=4097)) == -22 and both(yv=y(w=4097)) == -22
    assert L.prpe_roi_resize(None, p, p, 2, C.byref(y()), None, None) == -22
    assert L.prpe_roi_resize_u8(C.byref(fr), p, p, 2, None, a3, 0, C.byref(y()), None, None) == -22

    def match(meta_p=p, K=17, head=5, max_p=4, max_f=4, B=2, thr=0.3, status=p):
        return L.prpe_face_person_match(meta_p, p, max_p, p, K, p, p, max_f, p, p, thr, head, B, p, p, p, status, None)
    assert match(meta_p=None) == -22 and match(status=None) == -22
    assert match(head=0) == -22 and match(head=18) == -22 and match(K=4, head=5) == -22
    assert match(max_p=0) == -22 and match(max_f=0) == -22 and match(B=0) == -22 and match(thr=NAN) == -22


# ---------------------------------------------------------------------------------- host helpers
def test_ops_validate_arguments_before_any_launch():
    from prpe import ops
    for name in ("roi_select", "roi_resize", "roi_resize_u8", "face_person_match"):
        assert callable(getattr(ops, name))
    d, c = T._dets([[(0, 0, 30, 40, 0.9)]])
    meta, n = torch.zeros(4, 8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="dets"):
        ops.roi_select(d, c, (64, 64), (112, 112), crop_meta=meta, n_crops=n, status=n.clone())      # host tensors
    with pytest.raises(ValueError, match="dets"):
        ops.roi_select(d[..., :5], c, (64, 64), (112, 112), crop_meta=meta, n_crops=n, status=n.clone())
    with pytest.raises(ValueError, match="frames"):
        ops.roi_resize(torch.zeros(1, 3, 8, 8), meta, n, torch.zeros(4, 12, 12, 4))
    with pytest.raises(ValueError, match="frames"):
        ops.roi_resize_u8(torch.zeros(1, 8, 8, 3), meta, n, torch.zeros(4, 12, 12, 4))              # not uint8
    with pytest.raises(ValueError, match="crop_meta"):
        ops._roi_args("t", torch.zeros(4, 7), n, torch.zeros(4, 12, 12, 4), None)
    with pytest.raises(ValueError, match="crop_meta"):
        ops.face_person_match(torch.zeros(8), n, torch.zeros(4, 17, 3), meta, n, None, None, 1, face_slot=None,
                              person_ident=None, person_score=None, status=None)
    with pytest.raises(ValueError, match="keypoints"):
        ops.face_person_match(meta, n, torch.zeros(4, 17, 2), meta, n, None, None, 1, face_slot=None,
                              person_ident=None, person_score=None, status=None)


def test_constructors_refuse_what_the_stages_cannot_take():
    from prpe import FaceCrops, FaceGallery, PersonRecognition
    model = object()                                  # the constructors do not touch the model
    g = FaceGallery(dim=512, capacity=2, device="cpu")
    FaceCrops(model, g)
    FaceCrops(model)                                  # embeddings only
    with pytest.raises(ValueError, match="max_per_frame"):
        FaceCrops(model, g, max_per_frame=0)
    with pytest.raises(ValueError, match="max_crops"):
        FaceCrops(model, g, max_crops=0)
    with pytest.raises(ValueError, match="512"):
        FaceCrops(model, FaceGallery(dim=64, capacity=2, device="cpu"))
    with pytest.raises(ValueError, match="FaceGallery"):
        FaceCrops(model, gallery=torch.zeros(2, 512))
    with pytest.raises(ValueError, match="pad"):
        FaceCrops(model, g, pad=0.0)
    with pytest.raises(ValueError, match="pad"):
        FaceCrops(model, g, pad=NAN)
    pr = PersonRecognition(model, g, pose=dict(max_per_frame=32), faces=dict(max_per_frame=32))
    assert pr.pose.max_per_frame == pr.faces.max_per_frame == 32
    with pytest.raises(ValueError, match="at most 32"):
        PersonRecognition(model, g, pose=dict(max_per_frame=33))
    with pytest.raises(ValueError, match="at most 32"):
        PersonRecognition(model, g, faces=dict(max_per_frame=33))
    with pytest.raises(ValueError, match="person head"):
        PersonRecognition(model, g, pose=dict(branch="yolo_face"))
    with pytest.raises(ValueError, match="head_kpts"):
        PersonRecognition(model, g, head_kpts=0)
    with pytest.raises(ValueError, match="head_kpts"):
        PersonRecognition(model, g, head_kpts=18)


def test_face_stem_buffer_is_a_kind_of_its_own():
    """Engine.face_stem_buf does not share stem_buf's kind: alternating frames (batch B) and face
    crops (batch max_crops) keeps both buffers."""
    from prpe import engine as E
    e = E.Engine({}, device="cpu")
    a, b = e._batch_buf("stem_buf", 2, (64 + 6, 96 + 8, 4)), e.face_stem_buf(5)
    assert b.shape == (5, 118, 120, 4) and float(b.abs().max()) == 0.0
    assert e.face_stem_buf(5) is b and e._batch_buf("stem_buf", 2, (70, 104, 4)) is a and e.face_stem_buf(5) is b
    assert e.face_stem_buf(3) is not b and ("face_stem_buf", 5, 118, 120, 4) not in e._aux      # one batch size per kind
    assert ("stem_buf", 2, 70, 104, 4) in e._aux


def _face_out(frames_faces, cap):
    d, c = T._dets([[(*box, s) for box, s, _, _ in fs] for fs in frames_faces])
    meta, n, st = roi_select_ref(d, c, (112, 112), max_crops=cap)
    ident = torch.full((cap,), -1, dtype=torch.int64)
    score = torch.full((cap,), -INF)
    flat = [f for fs in frames_faces for f in fs]
    for s, (_, _, idn, sc) in enumerate(flat[:n]):
        ident[s], score[s] = idn, sc
    return {"dets": d, "counts": c, "crop_meta": meta, "n_crops": torch.tensor([n], dtype=torch.int32),
            "status": torch.tensor([st], dtype=torch.int32), "embeddings": torch.zeros(cap, 512),
            "norms": torch.zeros(cap), "ident": ident, "score": score}


def test_results_formatting():
    from prpe import FaceCrops, PersonRecognition
    big_id = (1 << 40) + 5                            # an int64 label survives the packed read
    out_f = _face_out([[((10, 20, 30, 40), 0.9, big_id, 0.75)], [], [((0, 0, 40, 20), 0.8, -1, 0.1),
                                                                      ((50, 50, 70, 70), 0.7, 3, 0.5)]], 5)
    faces = FaceCrops.results(out_f)
    assert [len(f) for f in faces] == [1, 0, 2]
    f0 = faces[0][0]
    assert f0["box"] == [7.5, 17.5, 32.5, 42.5] and f0["ident"] == big_id and f0["ident_score"] == 0.75
    assert f0["score"] == float(_f(0.9)) and f0["row"] == 0 and f0["slot"] == 0
    assert faces[2][1]["ident"] == 3 and faces[2][1]["slot"] == 2 and faces[2][0]["ident"] == -1

    d, c = T._dets([[(10, 20, 50, 120, 0.9)], [], [(0, 0, 120, 40, 0.8), (8, 16, 200, 272, 0.7)]])
    meta, n, st = T.select_ref(d, c, max_crops=4)
    kp = torch.zeros(4, 17, 3)
    kp[:n] = torch.arange(n * 51, dtype=torch.float32).view(n, 17, 3)
    out_p = {"dets": d, "counts": c, "crop_meta": meta, "n_crops": torch.tensor([n], dtype=torch.int32),
             "status": torch.tensor([st], dtype=torch.int32), "keypoints": kp}
    out = {"pose": out_p, "faces": out_f, "person_face": torch.tensor([0, -1, 2, -1], dtype=torch.int32),
           "person_ident": torch.tensor([big_id, -1, 3, -1]), "person_score": torch.tensor([0.75, -INF, 0.5, -INF]),
           "match_status": torch.zeros(3, dtype=torch.int32)}
    people = PersonRecognition.results(out)
    assert [len(p) for p in people] == [1, 0, 2]
    p = people[0][0]
    assert p["box"] == [-16.875, 7.5, -16.875 + 93.75, 7.5 + 125.0] and p["score"] == float(_f(0.9)) and p["row"] == 0
    assert p["ident"] == big_id and p["ident_score"] == 0.75 and p["face_box"] == [7.5, 17.5, 32.5, 42.5]
    assert torch.equal(p["keypoints"], kp[0])
    q = people[2][0]
    assert q["ident"] == -1 and q["ident_score"] == -INF and q["face_box"] is None
    r = people[2][1]
    assert r["ident"] == 3 and r["face_box"] == [47.5, 47.5, 72.5, 72.5] and r["row"] == 1
    assert torch.equal(r["keypoints"], kp[2])
