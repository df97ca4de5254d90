"""CPU: COCO keypoint AP / AR (prpe.evalsteps.CocoKeypointGT, csrc/cocoeval.hip) as far as the host
goes. pycocotools is not a dependency, so the yardstick is stated here twice: ``coco_eval_loop``
with COCOeval's own loop structure (per image, area range, threshold, detection, ground truth;
accumulate's cumulative sums and envelope loop), and ``coco_eval_masks``, written apart from it,
vectorised: OKS by broadcasting, the match by candidate masks instead of the ``break`` walk, AP
from an explicit precision-recall curve. Both must agree on every scenario; hand-worked cases pin
them to known values. tests/test_gpu_cocoeval.py holds the kernels to ``coco_eval_loop``."""
import functools
import json
import math

import numpy as np
import pytest

from prpe.evalsteps import (COCO_IOU_THRS, COCO_KP_AREA_RNGS, COCO_KP_SIGMAS, COCO_REC_THRS, CocoKeypointGT)

NAN = float("nan")
MD, MG, T, R, A = 20, 64, 10, 101, 3
EPS = np.spacing(1)
FAR = 1.0e6


def sigmas_for(K):
    return np.array([COCO_KP_SIGMAS[k % 17] for k in range(K)])


# ------------------------------------------------------------------ statement 1: COCOeval's loops
def _group(gt, dets):
    by = [[] for _ in gt.image_ids]
    for n, d in enumerate(dets):
        by[gt.row_of[int(d["image_id"])]].append(n)
    return by


def coco_eval_loop(gt, dets, sigmas=None):
    K = gt.K
    sigmas = sigmas_for(K) if sigmas is None else np.asarray(sigmas, dtype=np.float64)
    vars_ = (sigmas * 2) ** 2
    I = len(gt.image_ids)
    by = _group(gt, dets)
    kept, oks, evals = [], [], {}
    for r in range(I):
        g0, g1 = int(gt.gt_start[r]), int(gt.gt_start[r + 1])
        G = g1 - g0
        idx = by[r]
        sc = np.array([dets[n]["score"] for n in idx], dtype=np.float64)
        order = np.argsort(-sc, kind="mergesort")[:MD]
        kp = [idx[o] for o in order]
        kept.append(kp)
        D = len(kp)
        dkp = [np.array(dets[n]["keypoints"], dtype=np.float64) for n in kp]
        dscore = [float(dets[n]["score"]) for n in kp]
        darea = []
        for d in dkp:                                           # COCO.loadRes, keypoints
            x, y = d[0::3], d[1::3]
            darea.append((np.max(x) - np.min(x)) * (np.max(y) - np.min(y)))
        ious = np.zeros((D, G))                                 # COCOeval.computeOks
        for j in range(G):
            g = gt.kpts[g0 + j].reshape(-1)
            xg, yg, vg = g[0::3], g[1::3], g[2::3]
            k1 = np.count_nonzero(vg > 0)
            bb = gt.bbox[g0 + j]
            x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
            for i in range(D):
                xd, yd = dkp[i][0::3], dkp[i][1::3]
                if k1 > 0:
                    dx, dy = xd - xg, yd - yg
                else:
                    z = np.zeros(K)
                    dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                    dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
                e = (dx ** 2 + dy ** 2) / vars_ / (gt.area[g0 + j] + EPS) / 2
                if k1 > 0:
                    e = e[vg > 0]
                ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
        oks.append(ious)
        for a, (lo, hi) in enumerate(COCO_KP_AREA_RNGS):        # COCOeval.evaluateImg
            if G == 0 and len(idx) == 0:
                evals[r, a] = None
                continue
            g_ig = [bool(gt.ignore[g0 + j]) or gt.area[g0 + j] < lo or gt.area[g0 + j] > hi for j in range(G)]
            gtind = np.argsort(np.array(g_ig, dtype=np.uint8), kind="mergesort") if G else []
            gtm = np.zeros((T, G), dtype=np.int64)
            dtm = np.zeros((T, D), dtype=np.int64)
            dt_ig = np.zeros((T, D), dtype=bool)
            for ti, t in enumerate(COCO_IOU_THRS):
                for di in range(D):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gi in gtind:
                        if gtm[ti, gi] > 0 and not gt.iscrowd[g0 + gi]:
                            continue
                        if m > -1 and not g_ig[m] and g_ig[gi]:
                            break
                        if ious[di, gi] < iou:
                            continue
                        iou = ious[di, gi]
                        m = gi
                    if m == -1:
                        continue
                    dt_ig[ti, di] = g_ig[m]
                    dtm[ti, di] = 1 + m
                    gtm[ti, m] = 1 + di
            out = np.array([darea[i] < lo or darea[i] > hi for i in range(D)], dtype=bool).reshape(1, D)
            dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(out, T, 0)))
            evals[r, a] = {"scores": dscore, "dtm": dtm, "dt_ig": dt_ig, "g_ig": g_ig}
    precision = -np.ones((T, R, A))                             # COCOeval.accumulate
    recall = -np.ones((T, A))
    npig_img = np.zeros((I, A), dtype=np.int32)
    for a in range(A):
        E = [evals[r, a] for r in range(I) if evals[r, a] is not None]
        for r in range(I):
            if evals[r, a] is not None:
                npig_img[r, a] = sum(1 for v in evals[r, a]["g_ig"] if not v)
        if len(E) == 0:
            continue
        scores = np.concatenate([np.array(e["scores"], dtype=np.float64) for e in E])
        inds = np.argsort(-scores, kind="mergesort")
        dtm = np.concatenate([e["dtm"] for e in E], axis=1)[:, inds]
        dt_ig = np.concatenate([e["dt_ig"] for e in E], axis=1)[:, inds]
        npig = int(npig_img[:, a].sum())
        if npig == 0:
            continue
        tps = np.logical_and(dtm, np.logical_not(dt_ig))
        fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
        tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
        fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
        for ti, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
            tp, fp = np.array(tp), np.array(fp)
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + EPS)
            q = np.zeros((R,))
            recall[ti, a] = rc[-1] if nd else 0
            pr = pr.tolist()
            q = q.tolist()
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            pos = np.searchsorted(rc, COCO_REC_THRS, side="left")
            try:
                for ri, pi in enumerate(pos):
                    q[ri] = pr[pi]
            except IndexError:
                pass
            precision[ti, :, a] = np.array(q)
    stats = np.zeros(10)                                        # COCOeval.summarize, keypoints

    def summ(ap, ti=None, a=0):
        s = precision[:, :, a] if ap else recall[:, a]
        if ti is not None:
            s = s[ti:ti + 1]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    for k, ap in ((0, True), (5, False)):
        stats[k + 0], stats[k + 1], stats[k + 2] = summ(ap), summ(ap, 0), summ(ap, 5)
        stats[k + 3], stats[k + 4] = summ(ap, a=1), summ(ap, a=2)
    return {"kept": kept, "oks": oks, "evals": evals, "npig": npig_img, "precision": precision, "recall": recall,
            "stats": stats}


# ------------------------------------------------------------------ statement 2: masks and a PR curve
def coco_eval_masks(gt, dets, sigmas=None):
    K = gt.K
    sig = sigmas_for(K) if sigmas is None else np.asarray(sigmas, dtype=np.float64)
    var = (2.0 * sig) * (2.0 * sig)
    I = len(gt.image_ids)
    rows = np.array([gt.row_of[int(d["image_id"])] for d in dets], dtype=np.int64)
    score = np.array([d["score"] for d in dets], dtype=np.float64)
    allkp = np.array([d["keypoints"] for d in dets], dtype=np.float64).reshape(len(dets), K, 3)
    thr = np.minimum(COCO_IOU_THRS, 1 - 1e-10)
    rng = np.array(COCO_KP_AREA_RNGS, dtype=np.float64)
    ent_score, ent_m, ent_ig = [], [], []                        # per kept detection, image-major
    npig = np.zeros((I, A), dtype=np.int32)
    kept_all, oks_all = [], []
    for r in range(I):
        mine = np.flatnonzero(rows == r)
        s = score[mine]
        key = sorted(range(len(mine)), key=lambda i: (1, 0.0, i) if math.isnan(s[i]) else (0, -s[i], i))[:MD]
        kp = mine[key]
        kept_all.append([int(v) for v in kp])
        sl = slice(int(gt.gt_start[r]), int(gt.gt_start[r + 1]))
        g, area, bb = gt.kpts[sl], gt.area[sl], gt.bbox[sl]
        G, D = g.shape[0], len(kp)
        d = allkp[kp]
        vis = g[:, :, 2] > 0                                     # [G,K]
        none = ~vis.any(axis=1)                                  # bbox fallback rows
        dx = d[:, None, :, 0] - g[None, :, :, 0]
        dy = d[:, None, :, 1] - g[None, :, :, 1]
        lo_x, hi_x = (bb[:, 0] - bb[:, 2])[None, :, None], (bb[:, 0] + 2 * bb[:, 2])[None, :, None]
        lo_y, hi_y = (bb[:, 1] - bb[:, 3])[None, :, None], (bb[:, 1] + 2 * bb[:, 3])[None, :, None]
        fx = np.maximum(0, lo_x - d[:, None, :, 0]) + np.maximum(0, d[:, None, :, 0] - hi_x)
        fy = np.maximum(0, lo_y - d[:, None, :, 1]) + np.maximum(0, d[:, None, :, 1] - hi_y)
        dx = np.where(none[None, :, None], fx, dx)
        dy = np.where(none[None, :, None], fy, dy)
        e = (dx * dx + dy * dy) / var[None, None, :] / (area + EPS)[None, :, None] / 2
        use = np.where(none[:, None], True, vis)                 # [G,K]
        cnt = use.sum(axis=1)
        o = np.zeros((D, G))
        for i in range(D):
            for j in range(G):                                   # np.sum over the used terms only, as computeOks
                o[i, j] = np.sum(np.exp(-e[i, j][use[j]])) / cnt[j]
        oks_all.append(o)
        ext = (d[:, :, 0].max(axis=1) - d[:, :, 0].min(axis=1)) * (d[:, :, 1].max(axis=1) - d[:, :, 1].min(axis=1)) \
            if D else np.zeros(0)
        crowd = gt.iscrowd[sl].astype(bool)
        m_bits = np.zeros((D, A, T), dtype=bool)
        i_bits = np.zeros((D, A, T), dtype=bool)
        if G == 0 and len(mine) == 0:
            continue
        for a in range(A):
            ig = gt.ignore[sl].astype(bool) | (area < rng[a, 0]) | (area > rng[a, 1])
            npig[r, a] = int((~ig).sum())
            d_out = (ext < rng[a, 0]) | (ext > rng[a, 1])
            for t in range(T):
                taken = np.zeros(G, dtype=bool)
                for i in range(D):
                    cand = (~taken | crowd) & (o[i] >= thr[t]) if G else np.zeros(0, dtype=bool)
                    pick = -1
                    for group in (cand & ~ig, cand & ig):        # a non-ignored candidate wins over every ignored one
                        if group.any():
                            best = np.where(group, o[i], -np.inf)
                            pick = G - 1 - int(np.argmax(best[::-1]))   # the last of the best
                            break
                    if pick >= 0:
                        taken[pick] = True
                        m_bits[i, a, t] = True
                        i_bits[i, a, t] = ig[pick]
                    else:
                        i_bits[i, a, t] = d_out[i]
        ent_score.extend(score[kp].tolist())
        ent_m.extend(m_bits)
        ent_ig.extend(i_bits)
    precision = np.full((T, R, A), -1.0)
    recall = np.full((T, A), -1.0)
    n = len(ent_score)
    order = sorted(range(n), key=lambda i: (1, 0.0, i) if math.isnan(ent_score[i]) else (0, -ent_score[i], i))
    M = np.array(ent_m, dtype=bool).reshape(n, A, T)[order]
    Ig = np.array(ent_ig, dtype=bool).reshape(n, A, T)[order]
    for a in range(A):
        tot = int(npig[:, a].sum())
        if tot == 0:
            continue
        for t in range(T):
            tp = np.cumsum(M[:, a, t] & ~Ig[:, a, t]).astype(np.float64)
            fp = np.cumsum(~M[:, a, t] & ~Ig[:, a, t]).astype(np.float64)
            rc = tp / tot
            pr = tp / (fp + tp + EPS)
            env = np.maximum.accumulate(pr[::-1])[::-1] if n else pr     # the curve's upper envelope
            reach = rc[None, :] >= COCO_REC_THRS[:, None]         # [R,n]
            first = reach.argmax(axis=1) if n else np.zeros(R, dtype=np.int64)
            hit = reach.any(axis=1) if n else np.zeros(R, dtype=bool)
            precision[:, :, a][t] = np.where(hit, env[first] if n else 0.0, 0.0)
            recall[t, a] = rc[-1] if n else 0.0

    def mean_valid(v):
        v = v[v > -1]
        return -1.0 if v.size == 0 else float(np.sum(v) / v.size)
    stats = np.array([mean_valid(precision[:, :, 0]), mean_valid(precision[0, :, 0]), mean_valid(precision[5, :, 0]),
                      mean_valid(precision[:, :, 1]), mean_valid(precision[:, :, 2]),
                      mean_valid(recall[:, 0]), mean_valid(recall[0:1, 0]), mean_valid(recall[5:6, 0]),
                      mean_valid(recall[:, 1]), mean_valid(recall[:, 2])])
    return {"kept": kept_all, "oks": oks_all, "npig": npig, "precision": precision, "recall": recall, "stats": stats,
            "m": np.array(ent_m, dtype=bool).reshape(n, A, T), "ig": np.array(ent_ig, dtype=bool).reshape(n, A, T)}


# ------------------------------------------------------------------ the tables the kernels write
def tables(gt, ref):
    """``coco_eval_loop``'s result in prpe_coco_kp_match's layout: dt_rec [I,20] (index into the
    detection list = record index), dt_bits uint64 [I,20], npig [I,3], oks [I,20,64], dt_score."""
    I = len(gt.image_ids)
    rec = -np.ones((I, MD), dtype=np.int32)
    bits = np.full((I, MD), 1 << 63, dtype=np.uint64)
    oks = -np.ones((I, MD, MG))
    sc = np.zeros((I, MD))
    for r in range(I):
        kp = ref["kept"][r]
        rec[r, :len(kp)] = kp
        o = ref["oks"][r]
        oks[r, :o.shape[0], :o.shape[1]] = o
        for i in range(len(kp)):
            w = 0
            for a in range(A):
                ev = ref["evals"][r, a]
                for t in range(T):
                    w |= int(ev["dtm"][t, i] > 0) << (a * T + t)
                    w |= int(ev["dt_ig"][t, i]) << (A * T + a * T + t)
            bits[r, i] = w
            sc[r, i] = ref["evals"][r, 0]["scores"][i]
    return {"dt_rec": rec, "dt_bits": bits, "npig": ref["npig"], "oks": oks, "dt_score": sc}


def records_from_dets(dets, K):
    """Detection dicts (one image's in a row) as the record arrays prpe_pose_coco_records leaves:
    rec_kpts [n,K,3] fp32, rec_meta [n,8] fp32 (slot and instance as int32 bits, score), and the
    image id of every slot, in order of first appearance."""
    n = len(dets)
    kp = np.zeros((n, K, 3), dtype=np.float32)
    meta = np.zeros((n, 8), dtype=np.float32)
    slot_ids, seen = [], {}
    for r, d in enumerate(dets):
        i = int(d["image_id"])
        if i not in seen:
            seen[i] = len(slot_ids)
            slot_ids.append(i)
        kp[r] = np.asarray(d["keypoints"], dtype=np.float32).reshape(K, 3)
        meta[r, :2].view(np.int32)[:] = (seen[i], r)
        meta[r, 2] = d["score"]
    return kp, meta, slot_ids


def check_input_condition(ref):
    """No OKS within 1e-9 of a threshold, no two candidates of a detection within 1e-9 of each
    other, unless bit-equal by construction (the exact 0, 0.5, 1; duplicated ground truth): a 1-ulp
    exp must not be able to flip a match."""
    thr = np.minimum(COCO_IOU_THRS, 1 - 1e-10)
    for o in ref["oks"]:
        for row in o:
            for v in row:
                near = np.abs(v - thr) < 1e-9
                assert not near.any() or (v in (0.0, 0.5, 1.0) and (thr[near] == v).all()), (v, thr[near])
            s = np.sort(row[row >= thr[0] - 1e-9])             # below every threshold: never a candidate
            gap = np.diff(s)
            assert not ((gap < 1e-9) & (gap != 0)).any(), s


# ------------------------------------------------------------------ scenarios
def _f32(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def person(cx, cy, size, K=17, v=2):
    """K keypoints on a fixed pattern inside the size x size square centred at (cx, cy); values
    that fp32 holds exactly."""
    u = np.array([((7 * k + 3) % 16) / 16.0 for k in range(K)])
    w = np.array([((5 * k + 1) % 16) / 16.0 for k in range(K)])
    vis = np.full(K, v, dtype=np.float64) if np.isscalar(v) else np.asarray(v, dtype=np.float64)
    return np.stack([_f32(cx + size * (u - 0.5)), _f32(cy + size * (w - 0.5)), vis], axis=1)


def ann(image_id, kp, bbox=None, area=None, iscrowd=0, num_keypoints=None):
    kp = np.asarray(kp, dtype=np.float64)
    if bbox is None:
        x0, y0, x1, y1 = kp[:, 0].min(), kp[:, 1].min(), kp[:, 0].max(), kp[:, 1].max()
        bbox = [x0, y0, max(x1 - x0, 1.0), max(y1 - y0, 1.0)]
    return {"image_id": image_id, "category_id": 1, "keypoints": kp.reshape(-1).tolist(),
            "bbox": [float(v) for v in bbox], "area": float(bbox[2] * bbox[3] if area is None else area),
            "iscrowd": iscrowd, "num_keypoints": int((kp[:, 2] > 0).sum()) if num_keypoints is None else num_keypoints}


def det(image_id, kp, score):
    kp = np.asarray(kp, dtype=np.float64).copy()
    kp[:, 2] = 2
    return {"image_id": image_id, "category_id": 1, "keypoints": _f32(kp).reshape(-1).tolist(),
            "score": float(np.float32(score))}


def shifted(kp, dx, dy=0.0):
    out = np.array(kp, dtype=np.float64)
    out[:, 0] += dx
    out[:, 1] += dy
    return out


def hand_cases():
    """name -> (annotations, extra image ids, detections, K)."""
    c = {}
    g = person(100, 100, 48)
    c["A"] = ([ann(1, g, area=2500.0)], [], [det(1, g, 0.9)], 17)
    g1, g2 = person(100, 100, 48), person(400, 300, 48)
    c["B"] = ([ann(1, g1, area=2500.0), ann(1, g2, area=2500.0)], [],
              [det(1, shifted(g1, FAR), 0.9), det(1, g1, 0.8)], 17)
    g = np.array([[10.0, 10.0, 2], [30.0, 40.0, 2]])
    d = g.copy()
    d[1, 0] += FAR
    c["C"] = ([ann(1, g, bbox=[10, 10, 20, 30], area=2500.0)], [], [det(1, d, 0.9)], 2)
    crowd, solo = person(100, 100, 64), person(500, 500, 48)
    c["D"] = ([ann(1, crowd, area=4096.0, iscrowd=1), ann(1, solo, area=2500.0)], [],
              [det(1, shifted(crowd, 1.0), 0.9), det(1, shifted(crowd, -1.0), 0.8), det(1, solo, 0.7)], 17)
    # E: K = 1, OKS = exp(-d^2 / (2 var area)); the detection lies at OKS ~0.62 of the non-ignored
    # ground truth and ~0.92 of the crowd (both clear of every threshold)
    var, area = (2 * COCO_KP_SIGMAS[0]) ** 2, 2500.0
    d1 = math.sqrt(-math.log(0.62) * 2 * var * area)
    d2 = math.sqrt(-math.log(0.92) * 2 * var * area)
    ga, gb = np.array([[100.0, 100.0, 2]]), np.array([[100.0 + d1 + d2, 100.0, 2]])
    c["E"] = ([ann(1, ga, bbox=[80, 80, 50, 50], area=area), ann(1, gb, bbox=[80, 80, 50, 50], area=area, iscrowd=1)],
              [], [det(1, np.array([[100.0 + d1, 100.0, 2]]), 0.9)], 1)
    # F: num_keypoints == 0: distance to the doubled box [bx - bw, bx + 2 bw]; inside it OKS is 1
    blank = person(100, 100, 48, v=0)
    c["F"] = ([ann(1, blank, bbox=[76, 76, 48, 48], area=2304.0, num_keypoints=0), ann(1, person(600, 600, 48), area=2500.0)],
              [], [det(1, person(100, 100, 100), 0.9), det(1, person(300, 100, 48), 0.8), det(1, person(600, 600, 48), 0.7)], 17)
    # G: an unmatched detection whose keypoint extent (187.5^2) is outside medium
    c["G"] = ([ann(1, person(100, 100, 48), area=2500.0)], [],
              [det(1, person(700, 700, 200), 0.9), det(1, person(100, 100, 48), 0.8)], 17)
    c["H"] = ([ann(1, person(100, 100, 48), area=2500.0), ann(2, person(100, 100, 48), area=2500.0)], [],
              [det(1, person(100, 100, 48), 0.9)], 17)
    c["I"] = ([ann(1, person(100, 100, 48), area=2500.0)], [2],
              [det(2, person(100, 100, 48), 0.9), det(2, person(200, 100, 48), 0.8), det(1, person(100, 100, 48), 0.5)], 17)
    dj = [det(1, person(100 + 40 * n, 900, 48), 0.9 - 0.01 * n) for n in range(21)]
    dj[7] = det(1, person(100, 100, 48), 0.05)                   # the exact one is the 21st by score
    c["J"] = ([ann(1, person(100, 100, 48), area=2500.0)], [], dj, 17)
    # K: records of image 7 come first, image 3 sorts first; image 5: equal scores keep record order
    c["K"] = ([ann(3, person(100, 100, 48), area=2500.0), ann(7, person(100, 100, 48), area=2500.0)], [5],
              [det(7, person(100, 100, 48), 0.5), det(3, person(900, 900, 48), 0.5),
               det(5, person(100, 100, 48), 0.25), det(5, person(200, 200, 48), 0.25), det(5, person(300, 300, 48), 0.25)], 17)
    c["L"] = ([ann(1, person(100, 100, 48), area=2500.0)], [],
              [det(1, person(100, 100, 48), NAN), det(1, person(900, 900, 48), 0.1)], 17)
    return c


def random_epoch(seed, I, G_per, D_per, K, noise=(0.0, 0.5, 2.0, 6.0, 15.0, 40.0)):
    """I images; image r has G_per[r % len] persons and D_per[r % len] detections = its ground
    truth (cycled) + noise of graded size, scores and coordinates fp32-exact. Images are numbered
    from 11 in steps of 3 and the records come in descending image id."""
    rs = np.random.RandomState(seed)
    anns, dets, ids = [], [], []
    for r in range(I):
        iid = 11 + 3 * r
        ids.append(iid)
        G, D = G_per[r % len(G_per)], D_per[r % len(D_per)]
        people = []
        for j in range(G):
            size = float(rs.choice([24.0, 40.0, 64.0, 120.0, 200.0]))
            cx, cy = rs.uniform(50, 600, 2)
            vis = rs.choice([0, 1, 2], size=K, p=[0.2, 0.2, 0.6])
            kind = rs.rand()
            if kind < 0.1:
                vis[:] = 0
            kp = person(cx, cy, size, K, vis)
            kp[:, :2] = _f32(kp[:, :2] + rs.uniform(-0.2, 0.2, (K, 2)) * size)
            people.append(kp)
            anns.append(ann(iid, kp, bbox=[cx - size / 2, cy - size / 2, size, size],
                            area=float(size * size * rs.uniform(0.4, 0.9)), iscrowd=int(0.1 <= kind < 0.2),
                            num_keypoints=int((vis > 0).sum())))
        mine = []
        for n in range(D):
            if G:
                base = people[n % G]
                kp = base.copy()
                kp[:, :2] += rs.normal(0, 1, (K, 2)) * noise[(n // G + n) % len(noise)]
            else:
                kp = person(*rs.uniform(50, 600, 2), float(rs.choice([24.0, 80.0, 200.0])), K)
            score = float(rs.choice([rs.uniform(0.05, 1.0), 0.5, 0.25], p=[0.8, 0.1, 0.1]))
            mine.append(det(iid, kp, score))
        dets = mine + dets
    return anns, ids, dets, K


# (I, persons per image, detections per image, K): the smallest shapes at which a branch can go wrong
SHAPES = {
    "i1_g0_d1": (1, [0], [1], 17), "i1_g1_d0": (1, [1], [0], 17), "i1_g1_d1_k1": (1, [1], [1], 1),
    "i2_g2_d19_k2": (2, [2], [19], 2), "i1_g63_d20": (1, [63], [20], 17), "i1_g64_d21": (1, [64], [21], 17),
    "i2_g64_d40_k64": (2, [64, 1], [40, 20], 64), "i5_mixed": (5, [0, 1, 2, 0, 2], [0, 21, 40, 19, 1], 17),
    "i5_g1_d40_k1": (5, [1], [40], 1), "i2_empty": (2, [0], [0], 17),
}
SHAPE_SEEDS = {name: 100 + n for n, name in enumerate(sorted(SHAPES))}
EPOCH_SEED = 7


@functools.lru_cache(maxsize=None)
def scenario(name):
    """(gt, detections, K, coco_eval_loop's result), computed once and shared; never changed."""
    if name in SHAPES:
        I, Gs, Ds, K = SHAPES[name]
        anns, ids, dets, K = random_epoch(SHAPE_SEEDS[name], I, Gs, Ds, K)
    elif name == "epoch64":
        rs = np.random.RandomState(EPOCH_SEED)
        Gs = [int(v) for v in rs.randint(0, 7, 64)]
        Ds = [g + int(e) for g, e in zip(Gs, rs.randint(0, 3, 64))]
        anns, ids, dets, K = random_epoch(EPOCH_SEED, 64, Gs, Ds, 17)
    else:
        anns, ids, dets, K = hand_cases()[name]
    gt = CocoKeypointGT.from_annotations(anns, image_ids=ids, num_keypoints=K)
    return gt, dets, K, coco_eval_loop(gt, dets)


def scenario_names():
    return sorted(hand_cases()) + sorted(SHAPES) + ["epoch64"]


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", scenario_names())
def test_the_two_statements_agree(name):
    gt, dets, K, a = scenario(name)
    check_input_condition(a)
    b = coco_eval_masks(gt, dets)
    assert a["kept"] == b["kept"]
    assert np.array_equal(a["npig"], b["npig"])
    n = 0
    for r in range(len(gt)):
        assert np.array_equal(a["oks"][r], b["oks"][r])
        for i in range(len(a["kept"][r])):
            for ar in range(A):
                ev = a["evals"][r, ar]
                assert np.array_equal(ev["dtm"][:, i] > 0, b["m"][n, ar]), (r, i, ar)
                assert np.array_equal(ev["dt_ig"][:, i], b["ig"][n, ar]), (r, i, ar)
            n += 1
    assert np.array_equal(a["precision"], b["precision"])
    assert np.array_equal(a["recall"], b["recall"])
    assert np.abs(a["stats"] - b["stats"]).max() <= 1e-12


def _stats(name):
    return dict(zip(("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl"), scenario(name)[3]["stats"]))


def test_case_a_exact_detection():
    ref, s = scenario("A")[3], _stats("A")
    assert ref["oks"][0][0, 0] == 1.0
    one = 1.0 / (1.0 + EPS)                                     # pr = tp / (fp + tp + 2^-52)
    assert [s[k] for k in ("AP", "AP50", "AP75")] == pytest.approx([one] * 3, abs=1e-15)
    assert [s[k] for k in ("AR", "AR50", "AR75")] == [1.0] * 3
    assert (s["APm"], s["ARm"], s["APl"], s["ARl"]) == (pytest.approx(one, abs=1e-15), 1.0, -1.0, -1.0)   # area 2500: medium


def test_case_b_false_positive_ranked_first():
    ref, s = scenario("B")[3], _stats("B")
    ev = ref["evals"][0, 0]
    assert (ev["dtm"][0] > 0).tolist() == [False, True] and not ev["dt_ig"].any()
    assert s["AP50"] == pytest.approx(51 * 0.5 / 101, abs=1e-12) and s["AR"] == 0.5
    assert np.array_equal(ref["precision"][0, :51, 0], np.full(51, 1.0 / (1.0 + 1.0 + EPS)))
    assert not ref["precision"][0, 51:, 0].any()


def test_case_c_oks_on_the_threshold():
    ref = scenario("C")[3]
    assert ref["oks"][0][0, 0] == 0.5
    assert (ref["evals"][0, 0]["dtm"][:, 0] > 0).tolist() == [True] + [False] * 9


def test_case_d_crowd_absorbs_detections():
    ref, s = scenario("D")[3], _stats("D")
    ev = ref["evals"][0, 0]
    assert (ev["dtm"] > 0).all() and ev["dt_ig"][:, :2].all() and not ev["dt_ig"][:, 2].any()
    assert s["AP"] == pytest.approx(1.0, abs=1e-12)             # a false positive above it would halve this
    assert s["AR"] == 1.0


def test_case_e_break_rule_prefers_the_non_ignored():
    ref = scenario("E")[3]
    o = ref["oks"][0][0]
    assert abs(o[0] - 0.62) < 1e-4 and abs(o[1] - 0.92) < 1e-4
    ev = ref["evals"][0, 0]
    assert ev["dtm"][:, 0].tolist() == [1, 1, 1, 2, 2, 2, 2, 2, 2, 0]       # gt 1 while 0.62 reaches the threshold
    assert ev["dt_ig"][:, 0].tolist() == [False] * 3 + [True] * 6 + [False]


def test_case_f_no_keypoints_uses_the_box():
    ref = scenario("F")[3]
    o = ref["oks"][0]
    assert o[0, 0] == 1.0                                       # inside [bx - bw, bx + 2 bw]: distance 0
    assert 0.0 < o[1, 0] < 1.0
    ev = ref["evals"][0, 0]
    assert ev["g_ig"] == [True, False]
    assert ev["dtm"][0].tolist() == [1, 0, 2] and ev["dt_ig"][0].tolist() == [True, False, False]


def test_case_g_unmatched_outside_the_range():
    ref, s = scenario("G")[3], _stats("G")
    assert not (ref["evals"][0, 0]["dtm"][:, 0] > 0).any() and not ref["evals"][0, 0]["dt_ig"][:, 0].any()
    assert ref["evals"][0, 1]["dt_ig"][:, 0].all()
    assert s["APm"] == pytest.approx(1.0, abs=1e-12) and s["AP"] == pytest.approx(0.5, abs=1e-12)


def test_case_h_image_without_records_counts_as_misses():
    s = _stats("H")
    assert s["AR"] == 0.5 and s["AP"] == pytest.approx(51 / 101, abs=1e-12)


def test_case_i_image_without_ground_truth_gives_false_positives():
    ref, s = scenario("I")[3], _stats("I")
    assert ref["npig"].tolist() == [[1, 1, 0], [0, 0, 0]]
    assert s["AP"] == pytest.approx(1 / 3, abs=1e-12) and s["AR"] == 1.0


def test_case_j_the_21st_by_score_is_dropped():
    ref, s = scenario("J")[3], _stats("J")
    assert len(ref["kept"][0]) == 20 and 7 not in ref["kept"][0]
    assert s["AP"] == 0.0 and s["AR"] == 0.0


def test_case_k_equal_scores_keep_image_then_record_order():
    gt, dets, K, ref = scenario("K")
    assert gt.image_ids == [3, 5, 7] and ref["kept"] == [[1], [2, 3, 4], [0]]
    assert _stats("K")["AP50"] == pytest.approx(51 * 0.5 / 101, abs=1e-12)     # image 3's miss comes before image 7's hit


def test_case_l_nan_score_sorts_last():
    ref, s = scenario("L")[3], _stats("L")
    assert ref["kept"][0] == [1, 0]
    assert s["AP50"] == pytest.approx(0.5, abs=1e-12)           # the hit comes second; first it would give 1


def test_from_annotations_parses_plain_coco_json(tmp_path):
    anns = [ann(9, person(10, 10, 8), iscrowd=1), ann(4, person(30, 30, 8, v=0), num_keypoints=0),
            ann(9, person(50, 50, 8)), dict(ann(4, person(1, 1, 2)), category_id=3)]
    doc = {"images": [{"id": 12}, {"id": 4}, {"id": 9}], "annotations": anns}
    path = tmp_path / "person_keypoints.json"
    path.write_text(json.dumps(doc))
    for src in (str(path), doc):
        gt = CocoKeypointGT.from_annotations(src)
        assert gt.image_ids == [4, 9, 12] and gt.K == 17 and gt.max_gt == 2
        assert gt.gt_start.tolist() == [0, 1, 3, 3] and gt.gt_start.dtype == np.int32
        assert gt.iscrowd.tolist() == [0, 1, 0] and gt.ignore.tolist() == [1, 1, 0]
        assert np.array_equal(gt.kpts[1], person(10, 10, 8)) and gt.kpts.dtype == np.float64
        assert gt.bbox.shape == (3, 4) and gt.area.shape == (3,)
    gt = CocoKeypointGT.from_annotations(anns[:3], image_ids=[1])
    assert gt.image_ids == [1, 4, 9]
    assert gt.slot_to_img([9, 1, 9, 4]).tolist() == [2, 0, 2, 1]


def test_unknown_image_id_is_refused():
    gt = scenario("A")[0]
    with pytest.raises(ValueError, match="image id 5"):
        gt.slot_to_img([1, 5])


def test_more_than_64_persons_in_an_image_is_refused():
    anns = [ann(1, person(10 + n, 10, 8)) for n in range(65)]
    CocoKeypointGT.from_annotations(anns[:64])
    with pytest.raises(ValueError, match="65 annotations"):
        CocoKeypointGT.from_annotations(anns)


def test_constants_are_cocoeval_params():
    assert COCO_IOU_THRS.shape == (10,) and COCO_IOU_THRS[0] == 0.5 and COCO_IOU_THRS[5] == 0.75
    assert COCO_REC_THRS.shape == (101,) and COCO_REC_THRS[50] == 0.5 and (np.diff(COCO_REC_THRS) > 0).all()
    assert COCO_KP_AREA_RNGS == [[0, 1e10], [1024, 9216], [9216, 1e10]]
    assert COCO_KP_SIGMAS.dtype == np.float64 and COCO_KP_SIGMAS[0] == 0.26 / 10.0
