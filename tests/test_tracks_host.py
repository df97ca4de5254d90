"""CPU: tracking persons across frames (prpe.tracks, csrc/track.hip) as far as the host goes --
``track_update_ref``, a plain loop per stream, frame and pair on 0-dim float32 tensors written
from include/prpe.h alone (tests/test_gpu_tracks.py holds the kernel to it bit for bit), a second
statement on numpy float32 scalars written apart from it, the scenarios both tests share, hand
cases with literal numbers, the ABI table, the refusals and the host helpers of ``PersonTracker``."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import test_topdown_host as T
from prpe import _lib

NAN, INF = float("nan"), float("inf")
_f = T._f
SLOTS = 32
SIG = np.array([.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089],
               dtype=np.float32)
K2_17 = [float(v) for v in (np.float32(2) * SIG) * (np.float32(2) * SIG)]
DEFAULTS = dict(mode=0, gate=0.7, kp_thr=0.3, min_common=3, k2=None, new_thr=0.5, max_age=30)


def k2_for(K):
    return [K2_17[k % 17] for k in range(K)]


def fresh_state(S, K):
    meta = torch.zeros(S, SLOTS, 8)
    meta.view(torch.int32)[:, :, 0] = -1
    return {"trk_meta": meta, "trk_kpts": torch.zeros(S, SLOTS, K, 3),
            "trk_ident": torch.full((S, SLOTS), -1, dtype=torch.int64), "trk_iscore": torch.full((S, SLOTS), -INF),
            "next_id": torch.zeros(S, dtype=torch.int32)}


# ---------------------------------------------------------------------------------- the restatement
def _lt(a, b):
    return bool(a < b)


def iou_cost_ref(a, b):
    """mode 0 of include/prpe.h on (x0, y0, w, h) of the track ``a`` and the person ``b``."""
    a, b = [_f(v) for v in a], [_f(v) for v in b]
    ax1, ay1, bx1, by1 = a[0] + a[2], a[1] + a[3], b[0] + b[2], b[1] + b[3]
    ix = (bx1 if _lt(bx1, ax1) else ax1) - (b[0] if _lt(a[0], b[0]) else a[0])
    iy = (by1 if _lt(by1, ay1) else ay1) - (b[1] if _lt(a[1], b[1]) else a[1])
    ix = _f(0.0) if _lt(ix, 0) else ix
    iy = _f(0.0) if _lt(iy, 0) else iy
    inter = ix * iy
    uni = a[2] * a[3] + b[2] * b[3] - inter
    return _f(1.0) - inter / uni


def pose_cost_ref(win, tkp, dkp, kp_thr, min_common, k2):
    """mode 1: the cost, or None when fewer than min_common keypoints are common."""
    area = _f(win[2]) * _f(win[3])
    thr = _f(kp_thr)
    total, count = _f(0.0), 0
    for k in range(tkp.shape[0]):
        if bool(tkp[k, 2] >= thr) and bool(dkp[k, 2] >= thr):
            dx, dy = dkp[k, 0] - tkp[k, 0], dkp[k, 1] - tkp[k, 1]
            total = total + (dx * dx + dy * dy) / (area * _f(k2[k]))
            count += 1
    return total / _f(count) if count >= min_common else None


def track_update_ref(meta_p, n_p, kpts, ident, score, frame_stream, state, mode=0, gate=0.7, kp_thr=0.3,
                     min_common=3, k2=None, new_thr=0.5, max_age=30):
    """prpe_track_update on the host. Returns (track_id, track_hits, track_ident, track_iscore,
    status, state after the call); the state passed in is left as it is."""
    P, K = kpts.shape[:2]
    k2 = k2_for(K) if k2 is None else k2
    B = len(frame_stream)
    st = {k: v.clone() for k, v in state.items()}
    tm, ti = st["trk_meta"], st["trk_meta"].view(torch.int32)
    tk, tid, tis, nxt = st["trk_kpts"], st["trk_ident"], st["trk_iscore"], st["next_id"]
    S = tm.shape[0]
    pi = meta_p.view(torch.int32)
    n_p = max(0, min(int(n_p), P))
    o_id = torch.full((P,), -1, dtype=torch.int32)
    o_hits = torch.zeros(P, dtype=torch.int32)
    o_ident = torch.full((P,), -1, dtype=torch.int64)
    o_isc = torch.full((P,), -INF)
    status = torch.zeros(B, dtype=torch.int32)
    g, nt = _f(gate), _f(new_thr)
    for s in range(S):
        for b in range(B):
            if int(frame_stream[b]) != s:
                continue
            ps = [q for q in range(n_p) if int(pi[q, 0]) == b]
            if len(ps) > SLOTS:
                status[b] = 1
                continue
            live = [t for t in range(SLOTS) if int(ti[s, t, 0]) >= 0]
            cost = {}
            for t in live:
                for j, q in enumerate(ps):
                    if mode == 0:
                        c = iou_cost_ref(tm[s, t, 3:7], meta_p[q, 2:6])
                    else:
                        c = pose_cost_ref(tm[s, t, 3:7], tk[s, t], kpts[q], kp_thr, min_common, k2)
                    if c is not None and bool(torch.isfinite(c)) and bool(c <= g):
                        cost[(t, j)] = float(c)
            match = {}                                # person j -> track t
            while True:
                best = None
                for (t, j), c in cost.items():
                    if t not in match.values() and j not in match and (best is None or (c, t, j) < best):
                        best = (c, t, j)
                if best is None:
                    break
                match[best[2]] = best[1]

            def pair(q):
                carries = int(ident[q]) >= 0 and bool(torch.isfinite(score[q]))
                return (int(ident[q]), score[q].clone()) if carries else (-1, _f(-INF))

            for j, t in match.items():
                q = ps[j]
                tm[s, t, 3:7] = meta_p[q, 2:6]
                tm[s, t, 7] = meta_p[q, 6]
                tk[s, t] = kpts[q]
                ti[s, t, 1] = 0
                ti[s, t, 2] += 1
                idn, sc = pair(q)
                if idn >= 0:
                    if idn == int(tid[s, t]):
                        if bool(sc > tis[s, t]):
                            tis[s, t] = sc
                    elif bool(sc > tis[s, t]):
                        tid[s, t], tis[s, t] = idn, sc
            for t in live:
                if t not in match.values():
                    ti[s, t, 1] += 1
                    if int(ti[s, t, 1]) > max_age:
                        ti[s, t, 0], tid[s, t], tis[s, t] = -1, -1, -INF
            for j, q in enumerate(ps):
                if j in match or not bool(meta_p[q, 6] >= nt):
                    continue
                free = [t for t in range(SLOTS) if int(ti[s, t, 0]) < 0]
                if not free:
                    status[b] |= 2
                    continue
                t = free[0]
                ti[s, t, 0], ti[s, t, 1], ti[s, t, 2] = int(nxt[s]), 0, 1
                nxt[s] += 1
                tm[s, t, 3:7] = meta_p[q, 2:6]
                tm[s, t, 7] = meta_p[q, 6]
                tk[s, t] = kpts[q]
                tid[s, t], tis[s, t] = pair(q)
                match[j] = t
            for j, t in match.items():
                q = ps[j]
                o_id[q], o_hits[q], o_ident[q], o_isc[q] = ti[s, t, 0], ti[s, t, 2], tid[s, t], tis[s, t]
    return o_id, o_hits, o_ident, o_isc, status, st


# ---------------------------------------------------------------------------------- the second statement
def track_plain(meta_p, n_p, kpts, ident, score, frame_stream, state, mode=0, gate=0.7, kp_thr=0.3, min_common=3,
                k2=None, new_thr=0.5, max_age=30):
    """include/prpe.h's tracker once more, on numpy float32 scalars: frames in ascending b, each
    against the table of its own stream, association as one sorted walk over the eligible pairs.
    Written apart from ``track_update_ref`` and sharing no code with it."""
    f = np.float32
    mp = meta_p.numpy().copy()
    fr = mp.view(np.int32)[:, 0]
    kp = kpts.numpy()
    P, K = kp.shape[:2]
    k2 = np.array(k2_for(K) if k2 is None else k2, dtype=np.float32)
    idn, scs = ident.numpy(), score.numpy()
    M = state["trk_meta"].numpy().copy()
    ids, age, hits = (M.view(np.int32)[:, :, c] for c in range(3))
    TK = state["trk_kpts"].numpy().copy()
    TI, TS = state["trk_ident"].numpy().copy(), state["trk_iscore"].numpy().copy()
    NX = state["next_id"].numpy().copy()
    S, B = M.shape[0], len(frame_stream)
    n = min(max(int(n_p), 0), P)
    out = [np.full(P, -1, np.int32), np.zeros(P, np.int32), np.full(P, -1, np.int64), np.full(P, -np.inf, np.float32)]
    status = np.zeros(B, np.int32)

    def lo(u, v):
        return v if v < u else u

    def hi(u, v):
        return v if v > u else u

    with np.errstate(all="ignore"):
        for b in range(B):
            s = int(frame_stream[b])
            if not 0 <= s < S:
                continue
            slots = np.nonzero(fr[:n] == b)[0]
            if slots.size > 32:
                status[b] = 1
                continue
            was_live = [t for t in range(32) if ids[s, t] >= 0]
            pairs = []
            for t in was_live:
                ax, ay, aw, ah = (f(v) for v in M[s, t, 3:7])
                for q in slots:
                    bx, by, bw, bh = (f(v) for v in mp[q, 2:6])
                    if mode == 0:
                        ix = f(lo(f(ax + aw), f(bx + bw)) - hi(ax, bx))
                        iy = f(lo(f(ay + ah), f(by + bh)) - hi(ay, by))
                        ix, iy = (f(0) if ix < 0 else ix), (f(0) if iy < 0 else iy)
                        inter = f(ix * iy)
                        c = f(f(1) - f(inter / f(f(f(aw * ah) + f(bw * bh)) - inter)))
                    else:
                        common = [k for k in range(K) if TK[s, t, k, 2] >= f(kp_thr) and kp[q, k, 2] >= f(kp_thr)]
                        if len(common) < min_common:
                            continue
                        area, tot = f(aw * ah), f(0)
                        for k in common:
                            dx, dy = f(kp[q, k, 0] - TK[s, t, k, 0]), f(kp[q, k, 1] - TK[s, t, k, 1])
                            tot = f(tot + f(f(f(dx * dx) + f(dy * dy)) / f(area * k2[k])))
                        c = f(tot / f(len(common)))
                    if math.isfinite(c) and c <= f(gate):
                        pairs.append((float(c), t, int(q)))
            of = {}
            for c, t, q in sorted(pairs):
                if t not in of.values() and q not in of:
                    of[q] = t
            for q, t in of.items():
                M[s, t, 3:7], M[s, t, 7], TK[s, t] = mp[q, 2:6], mp[q, 6], kp[q]
                age[s, t] = 0
                hits[s, t] += 1
                if idn[q] >= 0 and math.isfinite(scs[q]):
                    if idn[q] == TI[s, t]:
                        TS[s, t] = scs[q] if scs[q] > TS[s, t] else TS[s, t]
                    elif scs[q] > TS[s, t]:
                        TI[s, t], TS[s, t] = idn[q], scs[q]
            for t in was_live:
                if t not in of.values():
                    age[s, t] += 1
                    if age[s, t] > max_age:
                        ids[s, t], TI[s, t], TS[s, t] = -1, -1, -np.inf
            fresh = [int(q) for q in slots if q not in of and mp[q, 6] >= f(new_thr)]
            free = [t for t in range(32) if ids[s, t] < 0]
            if len(fresh) > len(free):
                status[b] |= 2
            for q, t in zip(fresh, free):
                ids[s, t], age[s, t], hits[s, t] = NX[s], 0, 1
                NX[s] += 1
                M[s, t, 3:7], M[s, t, 7], TK[s, t] = mp[q, 2:6], mp[q, 6], kp[q]
                named = idn[q] >= 0 and math.isfinite(scs[q])
                TI[s, t], TS[s, t] = (idn[q], scs[q]) if named else (-1, -np.inf)
                of[q] = t
            for q, t in of.items():
                out[0][q], out[1][q], out[2][q], out[3][q] = ids[s, t], hits[s, t], TI[s, t], TS[s, t]
    new = {"trk_meta": M, "trk_kpts": TK, "trk_ident": TI, "trk_iscore": TS, "next_id": NX}
    return (*(torch.from_numpy(o) for o in out), torch.from_numpy(status), {k: torch.from_numpy(v) for k, v in new.items()})


# ---------------------------------------------------------------------------------- scenarios
def person(win, score=0.9, kp=None, ident=-1, iscore=-INF):
    """A person: window (x0, y0, w, h), detection score, keypoints ([(x, y, score)] * K, or None:
    K points on the window's diagonal with score 0.9), identity pair."""
    return (win, score, kp, ident, iscore)


def diag_kp(win, K, score=0.9):
    return [(win[0] + win[2] * (k + 1) / (K + 1), win[1] + win[3] * (k + 1) / (K + 1), score) for k in range(K)]


def build(frames, K, max_p=None, order=None, stale=True):
    """frames: per frame a list of persons -> (meta_p, n_p, kpts, ident, score) as PersonRecognition
    lays them out (ascending frame, then detection order), or in the slot ``order`` (a permutation
    of the filled slots); rows behind n_p are stale rows of a longer earlier list when ``stale``."""
    rows = [(b, *p) for b, ps in enumerate(frames) for p in ps]
    if order is not None:
        rows = [rows[i] for i in order]
    n = len(rows)
    P = max_p or n + 3
    meta = torch.zeros(P, 8)
    meta.view(torch.int32)[:, 0] = -1
    kp = torch.zeros(P, K, 3)
    ident = torch.full((P,), -1, dtype=torch.int64)
    score = torch.full((P,), -INF)
    for q, (b, win, sc, pts, idn, isc) in enumerate(rows):
        meta.view(torch.int32)[q, 0], meta.view(torch.int32)[q, 1] = b, q
        meta[q, 2:6] = torch.tensor(win, dtype=torch.float32)
        meta[q, 6] = sc
        kp[q] = torch.tensor(diag_kp(win, K) if pts is None else pts, dtype=torch.float32)
        ident[q], score[q] = idn, isc
    if stale:
        for q in range(n, P):
            meta.view(torch.int32)[q, 0] = q % max(len(frames), 1)
            meta[q, 2:7] = torch.tensor([0.0, 0.0, 50.0, 50.0, 0.99])
            kp[q, :, :] = torch.tensor([5.0, 5.0, 0.9])
            ident[q], score[q] = 999, 0.99
    return meta, n, kp, ident, score


def call(frames, frame_stream=None, K=17, S=1, **kw):
    fs = [b % S for b in range(len(frames))] if frame_stream is None else frame_stream
    return (*build(frames, K, **kw), torch.tensor(fs, dtype=torch.int32))


def _box(i, dx=0.0, size=20.0):
    """The i-th of a row of well separated 20 x 20 windows, moved by dx."""
    return (40.0 * (i % 8) + dx, 50.0 * (i // 8) + 0.5 * dx, size, size)


def _next(v, to):
    return float(torch.nextafter(_f(v), _f(to)))


@functools.lru_cache(maxsize=None)
def scenarios():
    """name -> (S, K, parameters, [calls]); a call = (meta_p, n_p, kpts, ident, score,
    frame_stream). The calls of a scenario run one after the other on one state, fresh at the start."""
    sc = {}
    far = (500.0, 500.0, 20.0, 20.0)
    # an empty state, slow motion, a person that leaves and one that arrives, n_p = 0, stale rows
    walk = [[person(_box(i, 2.0 * t)) for i in range(3)] for t in range(4)]
    walk[2] = walk[2][:2]                                            # person 2 is missed once
    walk[3] = walk[3] + [person(far)]
    sc["walk_iou"] = (1, 17, dict(), [call(walk[:2]), call([[]]), call(walk[2:]), call([[], []], max_p=4)])
    sc["walk_pose"] = (1, 17, dict(mode=1, gate=10.0), [call(walk[:2]), call(walk[2:])])
    # three streams interleaved over 40 frames and 70 slots, a frame of stream -1 and one of stream
    # S, stream 1 without a frame in the second call
    g = torch.Generator().manual_seed(7)
    fs = [b % 3 for b in range(40)]
    fs[5], fs[17] = -1, 3
    jit = (torch.rand(40, 2, generator=g) * 3).tolist()
    frames = [[person(_box(i + 2 * (fs[b] % 3), jit[b][i]), ident=(100 + i if b % 7 == 0 else -1), iscore=0.5 + 0.01 * b)
               for i in range(2 if b % 5 else 1)] for b in range(40)]
    assert sum(len(f) for f in frames) == 72
    frames[39] = []
    sc["three_streams"] = (3, 17, dict(), [call(frames, fs, S=3, max_p=70),
                                           call(frames[:6], [0, 2, 0, 2, 2, 0], S=3)])
    sc["three_streams_pose"] = (3, 17, dict(mode=1, gate=5.0, min_common=17), [call(frames, fs, S=3, max_p=70)])
    # capacity: 32 persons open 32 tracks, 32 against 32, a 33rd person (status 1: nothing moves,
    # nothing ages), a full table and a newcomer (status 2)
    full = [person(_box(i), score=0.6 + 0.01 * i) for i in range(32)]
    moved = [person(_box(i, 1.5), score=0.7) for i in range(32)]
    sc["capacity"] = (1, 2, dict(max_age=100, min_common=1), [call([full, moved], K=2, max_p=70),
                                                 call([moved + [person(far)]], K=2),
                                                 call([moved[:4] + [person(far)], [person(far)]], K=2)])
    # ties: person 0 overlaps tracks 0 and 1 alike (the lower track slot wins, track 1 ages); then
    # two persons overlap one track alike (the lower person slot wins, the other opens a track)
    sc["ties"] = (1, 17, dict(gate=0.9), [call([[person((0.0, 0.0, 10.0, 10.0)), person((20.0, 0.0, 10.0, 10.0))],
                                                 [person((5.0, 0.0, 20.0, 10.0))]]),
                                           call([[person((5.0, -5.0, 20.0, 10.0)), person((5.0, 5.0, 20.0, 10.0))]])])
    # the gate at equality and with the cost one float above it
    a, b = (0.0, 0.0, 30.0, 20.0), (7.0, 3.0, 30.0, 20.0)
    c = float(iou_cost_ref(a, b))
    for name, gate in (("gate_equal", c), ("gate_above", _next(c, -INF))):
        sc[name] = (1, 17, dict(gate=gate), [call([[person(a)], [person(b)]])])
    # degenerate geometry: zero-area windows (0 / 0), NaN and inf windows, then the tracks they left
    odd = [person((10.0, 10.0, 0.0, 0.0)), person((NAN, 0.0, 10.0, 10.0)), person((0.0, 0.0, INF, 10.0)),
           person((0.0, -INF, 10.0, 10.0)), person((60.0, 60.0, -10.0, 10.0)), person(_box(3))]
    sc["degenerate_iou"] = (1, 17, dict(), [call([odd, odd, odd])])
    kp = diag_kp(_box(0), 17)
    bad1, bad2 = list(kp), list(kp)
    bad1[4], bad2[6] = (NAN, kp[4][1], 0.9), (kp[6][0], INF, 0.9)
    nans = [person(_box(0), kp=bad1), person(_box(1), kp=[(x + 40.0, y, NAN) for x, y, _ in kp]),
            person(_box(2), kp=bad2), person((80.0, 0.0, 0.0, 20.0), kp=kp)]
    sc["degenerate_pose"] = (1, 17, dict(mode=1, gate=5.0), [call([nans, nans, nans])])
    # pose: exactly min_common common keypoints and one fewer; kp_thr at equality and one float below
    thr = float(_f(0.3))

    def some(n_good, score_good=0.9, shift=1.0):
        return [(x + shift, y, score_good if k < n_good else 0.1) for k, (x, y, _) in enumerate(kp)]
    sc["pose_common"] = (1, 17, dict(mode=1, gate=5.0, min_common=4),
                         [call([[person(_box(0), kp=kp), person(_box(1), kp=[(x + 40.0, y, s) for x, y, s in kp])],
                                [person(_box(0), kp=some(4)), person(_box(1), kp=[(x + 40.0, y, s) for x, y, s in some(3)])]])])
    sc["pose_thr"] = (1, 17, dict(mode=1, gate=5.0, min_common=17),
                      [call([[person(_box(0), kp=some(17, thr, 0.0)), person(_box(1), kp=[(x + 40.0, y, s) for x, y, s in kp])],
                             [person(_box(0), kp=kp),
                              person(_box(1), kp=[(x + 41.0, y, _next(thr, -INF) if k == 9 else 0.9) for k, (x, y, _) in enumerate(kp)])]])])
    for K in (1, 64):
        ppl = [[person(_box(i, 1.0 * t), kp=diag_kp(_box(i, 1.5 * t), K)) for i in range(3)] for t in range(3)]
        sc[f"pose_K{K}"] = (1, K, dict(mode=1, gate=5.0, min_common=1), [call(ppl, K=K)])
    # aging: max_age 0; the frame on which age reaches max_age and the next one; a slot freed in
    # step 4 and taken in step 5 of the same frame
    lone = [[person(_box(0))], [person(far)], [person(_box(0))]]
    sc["age_zero"] = (1, 17, dict(max_age=0), [call(lone)])
    sc["age_two"] = (1, 17, dict(max_age=2), [call([[person(_box(0)), person(_box(1))], [person(_box(1))], [person(_box(1))],
                                                      [person(_box(1, 1.0))], [person(_box(0)), person(_box(1))]])])
    # identity: new_thr at equality and one float below it; a name carried over five frames without
    # a face; replaced only by a strictly greater score; the same name keeps the greater score; a
    # NaN score names nobody
    nt = float(_f(0.5))
    sc["new_thr"] = (1, 17, dict(), [call([[person(_box(0), score=nt), person(_box(1), score=_next(nt, -INF))],
                                           [person(_box(0), score=0.1), person(_box(1), score=0.9)]])])
    named = [[person(_box(0, t), ident=(7 if t == 0 else -1), iscore=(0.6 if t == 0 else -INF))] for t in range(6)]
    rivals = [[person(_box(0, 6.0), ident=8, iscore=0.6)], [person(_box(0, 7.0), ident=8, iscore=_next(0.6, INF))],
              [person(_box(0, 8.0), ident=8, iscore=0.2)], [person(_box(0, 9.0), ident=8, iscore=0.9)],
              [person(_box(0, 10.0), ident=9, iscore=NAN)], [person(_box(0, 11.0), ident=9, iscore=INF)],
              [person(_box(1), ident=5, iscore=NAN)]]
    sc["identity"] = (1, 17, dict(), [call(named), call(rivals)])
    return sc


def run(fn, name):
    """The scenario's calls through ``fn`` (the signature of ``track_update_ref``) on one state:
    [(track_id, track_hits, track_ident, track_iscore, status, state after)] per call."""
    S, K, kw, calls = scenarios()[name]
    state, got = fresh_state(S, K), []
    for c in calls:
        got.append(fn(*c, state, **kw))
        state = got[-1][5]
    return got


@functools.lru_cache(maxsize=None)
def expected(name):
    return run(track_update_ref, name)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """Every output and every state array of two results of one call, bit for bit."""
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a[:5], b[:5])) \
        and all(torch.equal(bits(a[5][k]), bits(b[5][k])) for k in a[5])


@pytest.mark.parametrize("name", sorted(scenarios()))
def test_the_two_statements_agree(name):
    for want, got in zip(expected(name), run(track_plain, name)):
        assert same(want, got)


def _ids(res, n):
    return res[0][:n].tolist()


def test_scenarios_do_what_their_comments_say():
    """Literals worked out by hand from include/prpe.h, so that the scenarios test what they claim."""
    w = expected("walk_iou")
    assert _ids(w[0], 6) == [0, 1, 2, 0, 1, 2] and w[0][1][:6].tolist() == [1, 1, 1, 2, 2, 2]
    assert _ids(w[2], 6) == [0, 1, 0, 1, 2, 3]            # person 2 missed once, back with its id; a newcomer
    assert w[2][5]["trk_meta"].view(torch.int32)[0, 2, 1:3].tolist() == [0, 3] and int(w[3][5]["next_id"]) == 4
    assert w[3][5]["trk_meta"].view(torch.int32)[0, :4, 1].tolist() == [2, 2, 2, 2]       # two empty frames: all aged
    assert _ids(expected("walk_pose")[1], 6) == [0, 1, 0, 1, 2, 3]
    t = expected("three_streams")
    assert t[0][4].tolist() == [0] * 40
    frame = scenarios()["three_streams"][3][0][0].view(torch.int32)[:, 0]
    off = (frame == 5) | (frame == 17)                    # the frames of stream -1 and of stream S
    assert int(off.sum()) == 3 and bool((t[0][0][off] == -1).all()) and bool((t[0][0][~off] >= 0).all())
    assert t[0][5]["next_id"].tolist() == [2, 2, 2]
    cap = expected("capacity")
    assert sorted(_ids(cap[0], 32)) == list(range(32)) and _ids(cap[0], 64)[32:] == list(range(32))
    assert cap[1][4].tolist() == [1] and _ids(cap[1], 33) == [-1] * 33
    assert all(torch.equal(bits(cap[1][5][k]), bits(cap[0][5][k])) for k in cap[0][5])     # nothing moved, nothing aged
    assert cap[2][4].tolist() == [2, 2] and _ids(cap[2], 6) == [0, 1, 2, 3, -1, -1]
    assert cap[2][5]["trk_meta"].view(torch.int32)[0, :6, 1].tolist() == [1, 1, 1, 1, 2, 2]
    ties = expected("ties")
    assert _ids(ties[0], 3) == [0, 1, 0] and _ids(ties[1], 2) == [0, 2]
    assert _ids(expected("gate_equal")[0], 2) == [0, 0] and _ids(expected("gate_above")[0], 2) == [0, 1]
    d = expected("degenerate_iou")[0]
    assert _ids(d, 18) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 5, 11, 12, 13, 14, 15, 5]    # only the sound window matches
    dp = expected("degenerate_pose")[0]
    assert _ids(dp, 12) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]       # NaN / inf costs, NaN scores, area 0: no match
    assert _ids(expected("pose_common")[0], 4) == [0, 1, 0, 2]         # 4 common of min_common 4; 3: a new track
    assert _ids(expected("pose_thr")[0], 4) == [0, 1, 0, 2]            # score == kp_thr counts; one float below does not
    for K in (1, 64):
        assert _ids(expected(f"pose_K{K}")[0], 9) == [0, 1, 2] * 3
    assert _ids(expected("age_zero")[0], 3) == [0, 1, 2]
    az = expected("age_zero")[0][5]["trk_meta"].view(torch.int32)[0, :2, 0].tolist()
    assert az == [2, -1]                                  # freed in step 4, taken again in step 5 of the same frame
    assert _ids(expected("age_two")[0], 7) == [0, 1, 1, 1, 1, 2, 1]    # age 2 on the third frame, freed on the fourth
    assert _ids(expected("new_thr")[0], 4) == [0, -1, 0, 1]
    idn = expected("identity")
    assert idn[0][2][:6].tolist() == [7] * 6 and idn[0][1][:6].tolist() == [1, 2, 3, 4, 5, 6]
    assert idn[1][2][:7].tolist() == [7, 8, 8, 8, 8, 8, -1]
    assert [float(v) for v in idn[1][3][:6]] == [float(_f(0.6)), _next(0.6, INF), _next(0.6, INF)] + [float(_f(0.9))] * 3


def test_iou_cost_of_two_windows_with_iou_one_half():
    """a = (0, 0, 30, 20) and b = (10, 0, 30, 20): ix = 30 - 10 = 20, iy = 20, inter = 400,
    uni = 600 + 600 - 400 = 800, IoU = 0.5 exactly, c = 0.5. Disjoint windows: c = 1. The same
    window: c = 0. A zero-area pair: 0 / 0, not finite."""
    assert float(iou_cost_ref((0, 0, 30, 20), (10, 0, 30, 20))) == 0.5
    assert float(iou_cost_ref((0, 0, 30, 20), (40, 0, 30, 20))) == 1.0
    assert float(iou_cost_ref((3, 4, 30, 20), (3, 4, 30, 20))) == 0.0
    assert math.isnan(float(iou_cost_ref((5, 5, 0, 0), (5, 5, 0, 0))))


def test_pose_cost_of_one_displaced_keypoint():
    """K = 4 common keypoints, window 10 x 20 (area 200), k2 = 0.01 each; keypoint 2 is displaced
    by (3, 4): d_2 = 25 / (200 * 0.01) = 12.5 up to fp32 rounding of 0.01, the others 0; c = d_2 / 4.
    With keypoint 3 below kp_thr on one side the count is 3: c = d_2 / 3; min_common = 4: no cost."""
    tk = torch.tensor([[1.0, 1.0, 0.9], [2.0, 2.0, 0.9], [3.0, 3.0, 0.9], [4.0, 4.0, 0.9]])
    dk = tk.clone()
    dk[2, 0], dk[2, 1] = 6.0, 7.0
    d2 = _f(25.0) / (_f(200.0) * _f(0.01))
    assert abs(float(d2) - 12.5) < 1e-5
    assert float(pose_cost_ref((0, 0, 10, 20), tk, dk, 0.3, 4, [0.01] * 4)) == float(d2 / _f(4.0))
    dk[3, 2] = 0.1
    assert float(pose_cost_ref((0, 0, 10, 20), tk, dk, 0.3, 3, [0.01] * 4)) == float(d2 / _f(3.0))
    assert pose_cost_ref((0, 0, 10, 20), tk, dk, 0.3, 4, [0.01] * 4) is None


def test_identity_rule_three_branches():
    """A track named (7, 0.6) meets, frame by frame: the same name with 0.8 (the score rises), the
    same name with 0.5 (nothing), another name with 0.8 (not strictly greater: nothing), another
    name with 0.9 (replaced), nobody (kept)."""
    seq = [(7, 0.6), (7, 0.8), (7, 0.5), (8, 0.8), (8, 0.9), (-1, -INF)]
    frames = [[person(_box(0, float(t)), ident=i, iscore=s)] for t, (i, s) in enumerate(seq)]
    res = track_update_ref(*call(frames), fresh_state(1, 17))
    assert res[0][:6].tolist() == [0] * 6 and res[2][:6].tolist() == [7, 7, 7, 7, 8, 8]
    assert [float(v) for v in res[3][:6]] == [float(_f(v)) for v in (0.6, 0.8, 0.8, 0.8, 0.9, 0.9)]


# ---------------------------------------------------------------------------------- ABI
def test_abi_table_has_track_update_and_the_abi_is_still_12():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert _lib.ABI_VERSION == 12
    assert int(re.search(r"#define PRPE_ABI_VERSION (\d+)", header).group(1)) == 12
    decl = re.search(r"\bint prpe_track_update\s*\(([^;]*)\);", header)
    assert decl, "prpe_track_update is not declared in include/prpe.h"
    assert len(decl.group(1).split(",")) == 28 == len(_lib.SIGNATURES["prpe_track_update"][1])
    assert hasattr(_lib.lib(), "prpe_track_update") and _lib.lib().prpe_abi_version() == 12


def lib_refusals():
    """name -> keyword overrides of a valid call that the library must refuse with -EINVAL."""
    bad = {f"null_{i}": {"null": i} for i in range(17)}
    bad.update(B0=dict(B=0), S0=dict(S=0), K0=dict(K=0), P0=dict(max_p=0), K65=dict(K=65), mode2=dict(mode=2),
               mode_neg=dict(mode=-1), gate_nan=dict(gate=NAN), kp_thr_nan=dict(kp_thr=NAN), new_thr_nan=dict(new_thr=NAN),
               common0=dict(min_common=0), common_K1=dict(min_common=18), age_neg=dict(max_age=-1),
               k2_zero=dict(k2=[0.0] + K2_17[1:]), k2_neg=dict(k2=K2_17[:16] + [-1.0]), k2_nan=dict(k2=[NAN] + K2_17[1:]),
               k2_inf=dict(k2=K2_17[:5] + [INF] + K2_17[6:]))
    return bad


def lib_call(ptrs, B=2, S=1, K=17, max_p=4, mode=0, gate=0.7, kp_thr=0.3, min_common=3, k2=None, new_thr=0.5, max_age=30,
             null=None):
    """prpe_track_update on 16 device pointers ``ptrs`` (header order, k2 apart); ``null``: the
    index of the pointer to pass as NULL (16: k2)."""
    p = [None if i == null else v for i, v in enumerate(ptrs)]
    k2 = K2_17 if k2 is None else k2
    k2a = None if null == 16 else (C.c_float * len(k2))(*k2)
    return _lib.lib().prpe_track_update(p[0], p[1], max_p, p[2], K, p[3], p[4], p[5], B, S, mode, gate, kp_thr,
                                        min_common, k2a, new_thr, max_age, *p[6:16], None)


@pytest.mark.parametrize("name", sorted(lib_refusals()))
def test_library_rejects_bad_track_arguments_before_launch(name):
    assert lib_call([0x1000] * 16, **lib_refusals()[name]) == -22


# ---------------------------------------------------------------------------------- host helpers
def test_ops_validate_arguments_before_any_launch():
    from prpe import ops
    assert ops.TRACK_SLOTS == 32 and callable(ops.track_update)
    meta, n, kp = torch.zeros(4, 8), torch.zeros(1, dtype=torch.int32), torch.zeros(4, 17, 3)
    kw = dict(trk_meta=torch.zeros(1, 32, 8), trk_kpts=None, trk_ident=None, trk_iscore=None, next_id=None,
              track_id=None, track_hits=None, track_ident=None, track_iscore=None, status=None, k2=K2_17)
    fs = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="crop_meta_p"):
        ops.track_update(torch.zeros(8), n, kp, None, None, fs, **kw)
    with pytest.raises(ValueError, match="keypoints"):
        ops.track_update(meta, n, torch.zeros(4, 17, 2), None, None, fs, **kw)
    with pytest.raises(ValueError, match="frame_stream"):
        ops.track_update(meta, n, kp, None, None, [0, 0], **kw)
    with pytest.raises(ValueError, match="trk_meta"):
        ops.track_update(meta, n, kp, None, None, fs, **dict(kw, trk_meta=torch.zeros(32, 8)))
    with pytest.raises(ValueError, match="mode"):
        ops.track_update(meta, n, kp, None, None, fs, mode="oks", **kw)
    with pytest.raises(ValueError, match="crop_meta_p"):
        ops.track_update(meta, n, kp, None, None, fs, **kw)           # host tensors


def test_tracker_constructor_refuses_what_the_kernel_cannot_take():
    from prpe import FaceGallery, PersonRecognition, PersonTracker
    pr = PersonRecognition(object(), FaceGallery(dim=512, capacity=2, device="cpu"))
    t = PersonTracker(pr, n_streams=3, mode="pose")
    assert (t.n_streams, t.mode, t.gate, t.kp_thr, t.min_common, t.max_age) == (3, "pose", 1.0, 0.3, 3, 30)
    assert PersonTracker(pr).gate == 0.7 and t.k2 == K2_17
    t.reset()                                             # no state yet: nothing to do
    with pytest.raises(ValueError, match="PersonRecognition"):
        PersonTracker(object())
    for bad in (dict(n_streams=0), dict(mode="oks"), dict(gate=NAN), dict(kp_thr=NAN), dict(new_thr=NAN),
                dict(min_common=0), dict(min_common=18), dict(max_age=-1), dict(k2=[0.0] * 17), dict(k2=[1.0] * 65)):
        with pytest.raises(ValueError, match="PersonTracker"):
            PersonTracker(pr, **bad)


def test_tracker_state_reset_and_default_streams():
    """On host tensors: the fresh state is what include/prpe.h asks for, and reset(streams) refills
    those streams alone."""
    from prpe import FaceGallery, PersonRecognition, PersonTracker
    t = PersonTracker(PersonRecognition(object(), FaceGallery(dim=512, capacity=2, device="cpu")), n_streams=3)
    st = t._state(torch.device("cpu"))
    want = fresh_state(3, 17)
    assert all(torch.equal(bits(st[k]), bits(want[k])) for k in want)
    for v in st.values():
        v.view(torch.int32 if v.dtype != torch.int64 else torch.int64).fill_(5)
    t.reset([0, 2])
    for k in want:
        assert torch.equal(bits(st[k][[0, 2]]), bits(want[k][[0, 2]])), k
        assert bool((bits(st[k][1]) == 5).all()), k
    t.reset()
    assert all(torch.equal(bits(st[k]), bits(want[k])) for k in want)


def test_tracker_results_formatting():
    import test_faces_host as FH
    from prpe import PersonTracker
    big = (1 << 40) + 5
    out_f = FH._face_out([[((10, 20, 30, 40), 0.9, big, 0.75)], [], [((50, 50, 70, 70), 0.7, 3, 0.5)]], 5)
    d, c = T._dets([[(10, 20, 50, 120, 0.9)], [], [(0, 0, 120, 40, 0.8), (8, 16, 200, 272, 0.7)]])
    meta, n, st = T.select_ref(d, c, max_crops=4)
    kp = torch.arange(4 * 51, dtype=torch.float32).view(4, 17, 3)
    out_p = {"dets": d, "counts": c, "crop_meta": meta, "n_crops": torch.tensor([n], dtype=torch.int32),
             "status": torch.tensor([st], dtype=torch.int32), "keypoints": kp}
    out = {"pose": out_p, "faces": out_f, "person_face": torch.tensor([0, -1, 1, -1], dtype=torch.int32),
           "person_ident": torch.tensor([big, -1, 3, -1]), "person_score": torch.tensor([0.75, -INF, 0.5, -INF]),
           "match_status": torch.zeros(3, dtype=torch.int32),
           "track_id": torch.tensor([4, 0, -1, -1], dtype=torch.int32), "track_hits": torch.tensor([9, 1, 0, 0], dtype=torch.int32),
           "track_ident": torch.tensor([big, big + 1, -1, -1]), "track_ident_score": torch.tensor([0.8, 0.25, -INF, -INF]),
           "track_status": torch.zeros(3, dtype=torch.int32)}
    people = PersonTracker.results(out)
    assert [len(p) for p in people] == [1, 0, 2]
    a, b, c2 = people[0][0], people[2][0], people[2][1]
    assert (a["track_id"], a["track_hits"], a["track_ident"], a["track_ident_score"]) == (4, 9, big, float(_f(0.8)))
    assert a["ident"] == big and a["face_box"] == [7.5, 17.5, 32.5, 42.5] and torch.equal(a["keypoints"], kp[0])
    assert (b["track_id"], b["track_hits"], b["track_ident"], b["track_ident_score"]) == (0, 1, big + 1, 0.25)
    assert (c2["track_id"], c2["track_hits"], c2["track_ident"], c2["track_ident_score"]) == (-1, 0, -1, -INF)
    assert c2["ident"] == 3 and b["ident"] == -1
