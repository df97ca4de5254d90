"""CPU: annotated frames out (prpe.annotate, csrc/annotate.hip) as far as the host goes
-- the semantics of include/prpe.h restated twice: ``annotate_ref`` (numpy, int64 on pixel grids;
float32 for the one rounding), the yardstick tests/test_gpu_annotate.py holds the kernels to, and
``plain`` (a per-pixel, per-primitive loop on Python ints that shares no code with it), which agrees
with it on every small case below; hand-worked pixel sets; the palette helper; the ABI table and
every refusal of the library before a launch.

Every comparison is an equality: after one fp32 rounding per coordinate the feature is integers."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

from conftest import ROOT

from prpe import Annotator, NV12Frames, _lib, ops
from prpe import annotate as A

SLOT_MASK = 0x0FFFFFFF
Q_MIN, Q_MAX = -4096, 20479
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ cases
def case(B, H, W, persons=(), faces=(), K=17, limbs=ops.COCO_LIMBS, max_p=None, max_f=None, n_p=None, n_f=None,
         palette=None, box_t=2, limb_r=1, kp_r=2, kp_thr=0.3, cell=8, sx=1.0, sy=1.0):
    """A call's inputs as numpy arrays. ``persons``: (frame, (x0, y0, w, h), keypoints [K][3] or None,
    colour); ``faces``: (frame, (x0, y0, w, h), mode, colour). Rows past the lists hold stale values
    that would draw if they were read."""
    max_p = len(persons) if max_p is None else max_p
    max_f = len(faces) if max_f is None else max_f
    meta_p = np.zeros((max_p, 8), np.float32)
    kpts = np.zeros((max_p, K, 3), np.float32)
    pcol = np.zeros(max_p, np.int32)
    meta_p.view(np.int32)[:, 0] = 0
    meta_p[:, 2:6] = (1.0, 1.0, 9.0, 7.0)           # stale rows: a window that would be drawn
    kpts[:, :, :] = (3.0, 3.0, 1.0)
    for i, (frame, win, kp, col) in enumerate(persons):
        meta_p.view(np.int32)[i, 0] = frame
        meta_p[i, 2:6] = win
        kpts[i] = 0.0 if kp is None else np.asarray(kp, np.float32)
        pcol[i] = col
    meta_f = np.zeros((max_f, 8), np.float32)
    meta_f[:, 2:6] = (2.0, 2.0, 6.0, 6.0)
    fmode = np.full(max_f, 2, np.int32)
    fcol = np.zeros(max_f, np.int32)
    for i, (frame, win, mode, col) in enumerate(faces):
        meta_f.view(np.int32)[i, 0] = frame
        meta_f[i, 2:6] = win
        fmode[i], fcol[i] = mode, col
    if palette is None:
        palette = np.array([[200, 30, 40, 0], [90, 220, 10, 0], [15, 100, 250, 0], [255, 255, 0, 0], [1, 2, 3, 0]], np.uint8)
    return dict(B=B, H=H, W=W, K=K, meta_p=meta_p, n_p=len(persons) if n_p is None else n_p, kpts=kpts, pcol=pcol,
                meta_f=meta_f, n_f=len(faces) if n_f is None else n_f, fmode=fmode, fcol=fcol,
                palette=np.asarray(palette, np.uint8), limbs=tuple(limbs), box_t=box_t, limb_r=limb_r, kp_r=kp_r,
                kp_thr=kp_thr, cell=cell, sx=sx, sy=sy)


def surfaces(B, H, W, seed):
    """Random (y, uv, rgb) of one size: numpy uint8."""
    g = np.random.default_rng(seed)
    return (g.integers(0, 256, (B, H, W), dtype=np.uint8),
            g.integers(0, 256, (B, (H + 1) // 2, (W + 1) // 2, 2), dtype=np.uint8),
            g.integers(0, 256, (B, H, W, 3), dtype=np.uint8))


# ------------------------------------------------------------------ the restatement (numpy)
def _quant(v, s):
    """rintf(v * s) in float32, or None when the primitive is skipped."""
    with np.errstate(all="ignore"):
        r = np.rint(np.float32(v) * np.float32(s))
    if not (r >= Q_MIN and r <= Q_MAX):
        return None
    return int(r)


def _window(m, sx, sy):
    with np.errstate(all="ignore"):
        q = (_quant(m[2], sx), _quant(m[3], sy), _quant(np.float32(m[2]) + np.float32(m[4]), sx),
             _quant(np.float32(m[3]) + np.float32(m[5]), sy))
    if None in q or q[2] <= q[0] or q[3] <= q[1]:
        return None
    return q


def block_side(side, cell):
    return max(cell, 2 * ((side + 31) // 32))


def primitives(c):
    """[(frame, layer, slot, kind, (x0, y0, x1, y1), r)] of a case; layers 0 face, 1 box, 2 limb, 3 disc."""
    out = []
    n_p, n_f = (min(max(c[k], 0), len(c[m])) for k, m in (("n_p", "meta_p"), ("n_f", "meta_f")))
    for s in range(n_p):
        frame = int(c["meta_p"].view(np.int32)[s, 0])
        if not 0 <= frame < c["B"] or c["pcol"][s] < 0:
            continue
        if c["box_t"] > 0:
            w = _window(c["meta_p"][s], c["sx"], c["sy"])
            if w is not None:
                out.append((frame, 1, s, "outline", w, c["box_t"]))
        pts = []
        for j in range(c["K"]):
            x, y, sc = c["kpts"][s, j]
            q = (_quant(x, c["sx"]), _quant(y, c["sy"])) if sc >= np.float32(c["kp_thr"]) else (None, None)
            pts.append(None if None in q else q)
        for a, b in c["limbs"]:
            if pts[a] is not None and pts[b] is not None:
                out.append((frame, 2, s, "round", pts[a] + pts[b], c["limb_r"]))
        for q in pts:
            if q is not None:
                out.append((frame, 3, s, "round", q + q, c["kp_r"]))
    for s in range(n_f):
        frame = int(c["meta_f"].view(np.int32)[s, 0])
        if not 0 <= frame < c["B"] or c["fmode"][s] not in (1, 2):
            continue
        w = _window(c["meta_f"][s], c["sx"], c["sy"])
        if w is not None:
            out.append((frame, 0, s, "rect", w, 0))
    return out


def _covered(kind, q, r, X, Y):
    """Coverage of one primitive on int64 grids X, Y."""
    x0, y0, x1, y1 = q
    if kind == "round":
        pax, pay, pbx, pby = X - x0, Y - y0, X - x1, Y - y1
        dx, dy = x1 - x0, y1 - y0
        L2, dot, cr = dx * dx + dy * dy, pax * dx + pay * dy, dx * pay - dy * pax
        body = (dot >= 0) & (dot <= L2) & (cr * cr <= r * r * L2) if L2 > 0 else False
        return (pax * pax + pay * pay <= r * r) | (pbx * pbx + pby * pby <= r * r) | body
    inside = (X >= x0) & (X < x1) & (Y >= y0) & (Y < y1)
    if kind == "rect":
        return inside
    return inside & ~((X >= x0 + r) & (X < x1 - r) & (Y >= y0 + r) & (Y < y1 - r))


def keys_ref(c):
    """The winning key per pixel, int64 [B, H, W]: (layer + 1) << 28 | (SLOT_MASK - slot), 0: unpainted."""
    best = np.zeros((c["B"], c["H"], c["W"]), np.int64)
    Y, X = np.mgrid[0:c["H"], 0:c["W"]].astype(np.int64)
    for frame, layer, slot, kind, q, r in primitives(c):
        key = (layer + 1) << 28 | (SLOT_MASK - slot)
        np.maximum(best[frame], np.where(_covered(kind, q, r, X, Y), key, 0), out=best[frame])
    return best


def _mean(a):
    n = a.size
    return (int(a.astype(np.int64).sum()) + n // 2) // n


def _values(c, best, sample):
    """[B, H, W, 3] the three bytes of every painted pixel. ``sample(frame, ya, yb, xa, xb)`` -> the
    three block means of the original surface over that clipped block."""
    val = np.zeros(best.shape + (3,), np.uint8)
    n = len(c["palette"])
    for key in np.unique(best[best > 0]):
        layer, slot = (int(key) >> 28) - 1, SLOT_MASK - (int(key) & SLOT_MASK)
        where = best == key
        if layer > 0:
            val[where] = c["palette"][int(c["pcol"][slot]) % n, :3]
        elif c["fmode"][slot] == 2:
            val[where] = c["palette"][int(c["fcol"][slot]) % n, :3]
        else:
            x0, y0, x1, y1 = _window(c["meta_f"][slot], c["sx"], c["sy"])
            side = block_side(max(x1 - x0, y1 - y0), c["cell"])
            ax, ay = x0 & ~1, y0 & ~1
            for b, i, j in zip(*np.nonzero(where)):
                by, bx = (i - ay) // side, (j - ax) // side
                ya, yb = max(ay + by * side, 0), min(ay + (by + 1) * side, c["H"])
                xa, xb = max(ax + bx * side, 0), min(ax + (bx + 1) * side, c["W"])
                val[b, i, j] = sample(b, ya, yb, xa, xb)
    return val


def annotate_u8_ref(c, img):
    """prpe_annotate_u8 on img [B, H, W, 3] uint8 -> (the painted frames, the painted mask)."""
    best = keys_ref(c)
    val = _values(c, best, lambda b, ya, yb, xa, xb: [_mean(img[b, ya:yb, xa:xb, k]) for k in range(3)])
    out = img.copy()
    out[best > 0] = val[best > 0]
    return out, best > 0


def annotate_nv12_ref(c, y, uv):
    """prpe_annotate_nv12 on y [B, H, W], uv [B, ceil(H/2), ceil(W/2), 2] -> (y, uv, the painted luma mask)."""
    best = keys_ref(c)

    def sample(b, ya, yb, xa, xb):                   # ya and xa are even: pairs whose first pixel is in the block
        pairs = uv[b, ya // 2:(yb + 1) // 2, xa // 2:(xb + 1) // 2]
        return [_mean(y[b, ya:yb, xa:xb]), _mean(pairs[..., 0]), _mean(pairs[..., 1])]
    val = _values(c, best, sample)
    m = best > 0
    yo, uvo = y.copy(), uv.copy()
    yo[m] = val[..., 0][m]
    mc = m[:, ::2, ::2]
    uvo[mc] = val[:, ::2, ::2, 1:][mc]
    return yo, uvo, m


# ------------------------------------------------------------------ the plain statement (Python ints)
def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _q_plain(v, s):
    t = float(v) * float(s)                          # two float32 values: the fp64 product is exact
    if t != t or t in (INF, -INF):
        return None
    t = _f32(t)
    if t in (INF, -INF):
        return None
    r = round(t)                                     # half to even
    return r if Q_MIN <= r <= Q_MAX else None


def plain(c, planes):
    """The header's rules pixel by pixel: for every pixel the covering primitive of the highest layer
    and lowest slot, found by walking the layers from the top. ``planes``: ("u8", img) or
    ("nv12", y, uv). Returns the painted copies."""
    B, H, W, n = c["B"], c["H"], c["W"], len(c["palette"])
    sx, sy = _f32(c["sx"]), _f32(c["sy"])
    thr = _f32(c["kp_thr"])

    def win(m):
        xs, ys = _f32(float(m[2]) + float(m[4])), _f32(float(m[3]) + float(m[5]))
        w = [_q_plain(m[2], sx), _q_plain(m[3], sy), _q_plain(xs, sx), _q_plain(ys, sy)]
        return None if None in w or w[2] <= w[0] or w[3] <= w[1] else w

    def disc(px, py, cx, cy, r):
        return (px - cx) ** 2 + (py - cy) ** 2 <= r * r

    def seg(px, py, a, b, r):
        if disc(px, py, a[0], a[1], r) or disc(px, py, b[0], b[1], r):
            return True
        dx, dy = b[0] - a[0], b[1] - a[1]
        L2 = dx * dx + dy * dy
        if L2 == 0:
            return False
        t = (px - a[0]) * dx + (py - a[1]) * dy
        return 0 <= t <= L2 and (dx * (py - a[1]) - dy * (px - a[0])) ** 2 <= r * r * L2

    people, masks = [], []
    for s in range(min(max(c["n_p"], 0), len(c["meta_p"]))):
        f = int(c["meta_p"].view(np.int32)[s, 0])
        if not 0 <= f < B or c["pcol"][s] < 0:
            continue
        pts = []
        for j in range(c["K"]):
            x, y, sc = (float(v) for v in c["kpts"][s, j])
            q = (_q_plain(x, sx), _q_plain(y, sy)) if sc >= thr else (None, None)
            pts.append(None if None in q else q)
        people.append((s, f, win(c["meta_p"][s]) if c["box_t"] > 0 else None, pts))
    for s in range(min(max(c["n_f"], 0), len(c["meta_f"]))):
        f = int(c["meta_f"].view(np.int32)[s, 0])
        w = win(c["meta_f"][s])
        if 0 <= f < B and c["fmode"][s] in (1, 2) and w is not None:
            masks.append((s, f, w))

    def winner(f, px, py):
        for s, pf, _, pts in people:                 # discs
            if pf == f and any(q is not None and disc(px, py, q[0], q[1], c["kp_r"]) for q in pts):
                return ("person", s)
        for s, pf, _, pts in people:                 # limbs
            if pf == f and any(pts[a] is not None and pts[b] is not None and seg(px, py, pts[a], pts[b], c["limb_r"])
                               for a, b in c["limbs"]):
                return ("person", s)
        t = c["box_t"]
        for s, pf, w, _ in people:                   # outlines
            if pf == f and w is not None and w[0] <= px < w[2] and w[1] <= py < w[3] and \
                    not (w[0] + t <= px < w[2] - t and w[1] + t <= py < w[3] - t):
                return ("person", s)
        for s, ff, w in masks:
            if ff == f and w[0] <= px < w[2] and w[1] <= py < w[3]:
                return ("face", s, w)
        return None

    def mean(vals):
        return (sum(vals) + len(vals) // 2) // len(vals)

    src = [p.copy() for p in planes[1:]]
    dst = [p.copy() for p in planes[1:]]
    for f in range(B):
        for py in range(H):
            for px in range(W):
                hit = winner(f, px, py)
                if hit is None:
                    continue
                if hit[0] == "person":
                    v = [int(k) for k in c["palette"][int(c["pcol"][hit[1]]) % n, :3]]
                elif c["fmode"][hit[1]] == 2:
                    v = [int(k) for k in c["palette"][int(c["fcol"][hit[1]]) % n, :3]]
                else:
                    w = hit[2]
                    side = max(c["cell"], 2 * ((max(w[2] - w[0], w[3] - w[1]) + 31) // 32))
                    ax, ay = w[0] - (w[0] % 2), w[1] - (w[1] % 2)
                    bx, by = ax + (px - ax) // side * side, ay + (py - ay) // side * side
                    cells = [(i, j) for i in range(max(by, 0), min(by + side, H)) for j in range(max(bx, 0), min(bx + side, W))]
                    if planes[0] == "u8":
                        v = [mean([int(src[0][f, i, j, k]) for i, j in cells]) for k in range(3)]
                    else:
                        pairs = [(i // 2, j // 2) for i, j in cells if i % 2 == 0 and j % 2 == 0]
                        v = [mean([int(src[0][f, i, j]) for i, j in cells])] + \
                            [mean([int(src[1][f, i, j, k]) for i, j in pairs]) for k in range(2)]
                if planes[0] == "u8":
                    dst[0][f, py, px] = v
                else:
                    dst[0][f, py, px] = v[0]
                    if py % 2 == 0 and px % 2 == 0:
                        dst[1][f, py // 2, px // 2] = v[1:]
    return dst


# ------------------------------------------------------------------ small cases both statements take
def _kp(pts, K=17):
    k = np.zeros((K, 3), np.float32)
    for j, p in pts.items():
        k[j] = p
    return k


def small_cases():
    k1 = _kp({5: (3.0, 4.0, 0.9), 6: (14.0, 4.0, 0.9), 7: (3.0, 12.0, 0.3), 9: (9.0, 12.0, 0.29), 0: (8.5, 2.5, 1.0),
              11: (NAN, 3.0, 1.0), 12: (15.0, 11.0, NAN)})
    k2 = _kp({5: (10.0, 1.0, 0.8), 7: (16.0, 9.0, 0.8), 6: (-3.0, 6.0, 0.8), 8: (4.0, 13.0, 0.7)})
    return {
        "skeleton": case(2, 15, 19, persons=[(0, (1.0, 1.0, 15.0, 12.0), k1, 0), (0, (6.5, 0.0, 20.0, 9.5), k2, 6),
                                              (1, (2.0, 3.0, 5.0, 5.0), k2, -1), (1, (0.0, 0.0, 4.0, 30.0), None, 2),
                                              (2, (1.0, 1.0, 5.0, 5.0), k1, 1), (-1, (1.0, 1.0, 5.0, 5.0), k1, 1)]),
        "faces": case(2, 14, 17, persons=[(0, (2.0, 2.0, 9.0, 9.0), _kp({0: (6.0, 6.0, 1.0)}), 1)],
                      faces=[(0, (3.0, 1.0, 9.0, 7.0), 1, 0), (0, (7.0, 4.0, 8.0, 8.0), 2, 3), (1, (-3.0, 9.0, 9.0, 9.0), 1, 0),
                             (1, (11.0, 2.0, 1.0, 1.0), 1, 0), (1, (5.0, 5.0, 4.0, 4.0), 0, 0), (0, (1.0, 9.0, 5.0, 4.0), 2, 12)],
                      cell=2),
        "stale": case(1, 9, 11, persons=[(0, (1.0, 1.0, 6.0, 6.0), None, 0)], faces=[(0, (2.0, 2.0, 5.0, 5.0), 2, 1)],
                      max_p=3, max_f=3),
        "scaled": case(1, 13, 16, persons=[(0, (1.0, 0.5, 5.0, 3.5), _kp({5: (1.5, 1.25, 1.0), 6: (4.5, 3.75, 1.0)}), 1)],
                       faces=[(0, (2.5, 0.5, 2.5, 2.5), 1, 0)], sx=2.5, sy=3.0, cell=4, limb_r=0, kp_r=1),
        "thick": case(1, 10, 12, persons=[(0, (1.0, 1.0, 9.0, 5.0), None, 2)], box_t=3),
    }


@pytest.mark.parametrize("name", sorted(small_cases()))
def test_the_two_statements_agree(name):
    c = small_cases()[name]
    y, uv, img = surfaces(c["B"], c["H"], c["W"], 5)
    got, mask = annotate_u8_ref(c, img)
    assert np.array_equal(got, plain(c, ("u8", img))[0])
    gy, guv, m = annotate_nv12_ref(c, y, uv)
    py, puv = plain(c, ("nv12", y, uv))
    assert np.array_equal(gy, py) and np.array_equal(guv, puv)
    assert np.array_equal(mask, m) and mask.any()


# ------------------------------------------------------------------ hand-worked cases
def _painted(c):
    return {(int(j), int(i)) for _, i, j in zip(*np.nonzero(keys_ref(c) > 0))}


def _one_person(kp, **kw):
    return case(1, 12, 12, persons=[(0, (0.0, 0.0, 1.0, 1.0), _kp(kp), 0)], **{"box_t": 0, **kw})


def test_radius_1_disc_is_5_pixels():
    c = _one_person({0: (5.0, 6.0, 1.0)}, limbs=(), kp_r=1)
    assert _painted(c) == {(5, 6), (4, 6), (6, 6), (5, 5), (5, 7)}


def test_horizontal_and_diagonal_segments():
    c = _one_person({0: (2.0, 3.0, 1.0), 1: (6.0, 3.0, 1.0)}, limbs=((0, 1),), limb_r=0, kp_thr=0.5, kp_r=0)
    assert _painted(c) == {(x, 3) for x in range(2, 7)}
    c = _one_person({0: (2.0, 3.0, 1.0), 1: (6.0, 3.0, 1.0)}, limbs=((0, 1),), limb_r=1, kp_r=0)
    assert _painted(c) == {(x, y) for x in range(2, 7) for y in (2, 3, 4)} | {(1, 3), (7, 3)}      # round caps
    c = _one_person({0: (2.0, 2.0, 1.0), 1: (5.0, 5.0, 1.0)}, limbs=((0, 1),), limb_r=0, kp_r=0)
    assert _painted(c) == {(2, 2), (3, 3), (4, 4), (5, 5)}
    # radius 1 around the diagonal: cross^2 <= 1 * 18 -> |dx - dy| <= 1 (cross = 3 (dy - dx)), between the caps
    c = _one_person({0: (2.0, 2.0, 1.0), 1: (5.0, 5.0, 1.0)}, limbs=((0, 1),), limb_r=1, kp_r=0)
    want = {(t, t) for t in range(2, 6)} | {(t + 1, t) for t in range(2, 5)} | {(t, t + 1) for t in range(2, 5)}
    assert _painted(c) == want | {(1, 2), (2, 1), (6, 5), (5, 6)}
    # L2 = 0 is a disc
    c = _one_person({0: (4.0, 4.0, 1.0), 1: (4.0, 4.0, 1.0)}, limbs=((0, 1),), limb_r=1, kp_r=0)
    assert _painted(c) == {(4, 4), (3, 4), (5, 4), (4, 3), (4, 5)}


def test_thickness_2_outline():
    c = case(1, 12, 12, persons=[(0, (2.0, 3.0, 7.0, 6.0), None, 0)], box_t=2)
    want = {(x, y) for x in range(2, 9) for y in range(3, 9)} - {(x, y) for x in range(4, 7) for y in range(5, 7)}
    assert _painted(c) == want
    c = case(1, 12, 12, persons=[(0, (2.0, 3.0, 4.0, 6.0), None, 0)], box_t=2)        # nothing is left inside
    assert _painted(c) == {(x, y) for x in range(2, 6) for y in range(3, 9)}


def test_rounding_is_half_to_even_after_one_fp32_multiply():
    assert [_quant(v, 1.0) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 3.4999998)] == [0, 2, 2, 0, -2, 3]
    assert _quant(1.0, 2.5) == 2 and _quant(3.0, 0.5) == 2 and _quant(5.0, 0.5) == 2
    assert _quant(20479.0, 1.0) == 20479 and _quant(20479.5, 1.0) is None and _quant(-4096.5, 1.0) == -4096
    assert _quant(-4097.0, 1.0) is None and _quant(NAN, 1.0) is None and _quant(INF, 1.0) is None
    assert _quant(3e38, 2.0) is None
    for v, s in ((0.5, 1.0), (2.5, 1.0), (1.0, 2.5), (20479.5, 1.0), (NAN, 1.0), (3e38, 2.0), (7.3, 1.7)):
        assert _q_plain(np.float32(v), _f32(s)) == _quant(v, s)
    # the far edge: the fp32 sum first. 0.3f + 0.2f = 0.5 exactly in fp32 -> 0.5 * 1 -> 0 (an empty window)
    assert _window(np.array([0, 0, 0.3, 0.3, 0.2, 0.2], np.float32), 1.0, 1.0) is None
    assert _window(np.array([0, 0, 1.5, 2.5, 2.0, 2.0], np.float32), 1.0, 1.0) == (2, 2, 4, 4)


def test_pixelation_mean_with_odd_n_and_the_block_side():
    assert [block_side(s, 2) for s in (32, 33, 1000)] == [2, 4, 64] and block_side(1000, 64) == 64
    assert block_side(40, 8) == 8 and block_side(24575, 2) == 1536
    # a 3 x 3 face at (4, 4) of a 7 x 7 frame, cell 4: anchor (4, 4), one block of 4 x 4 that the frame
    # clips to 3 x 3, n = 9: five pixels of 11 among 10s sum to 95, (95 + 4) / 9 = 11; four give (94 + 4) / 9 = 10
    img = np.full((1, 7, 7, 3), 10, np.uint8)
    img[0, 4, 4:7, 0] = 11
    img[0, 5, 4:6, 0] = 11
    img[0, 4, 4:7, 1] = 11
    img[0, 5, 4, 1] = 11
    c = case(1, 7, 7, faces=[(0, (4.0, 4.0, 3.0, 3.0), 1, 0)], cell=4)
    out, mask = annotate_u8_ref(c, img)
    assert mask.sum() == 9 and out[0, 5, 5].tolist() == [11, 10, 10] and np.array_equal(out[~mask], img[~mask])
    # the block is not clipped to the window: a 3 x 3 face at the origin averages the 4 x 4 block
    img[0, 3, 3] = (255, 255, 255)
    c = case(1, 7, 7, faces=[(0, (0.0, 0.0, 3.0, 3.0), 1, 0)], cell=4)
    out, mask = annotate_u8_ref(c, img)
    assert mask.sum() == 9 and out[0, 0, 0].tolist() == [(15 * 10 + 255 + 8) // 16] * 3 == [25] * 3
    # NV12: luma over the 9 pixels, chroma over the 4 pairs whose first pixel is in the block
    y = np.full((1, 7, 7), 10, np.uint8)
    uv = np.full((1, 4, 4, 2), 100, np.uint8)
    uv[0, 2, 2] = (103, 101)
    uv[0, 3, 3] = (100, 102)
    c = case(1, 7, 7, faces=[(0, (4.0, 4.0, 3.0, 3.0), 1, 0)], cell=4)
    yo, uvo, m = annotate_nv12_ref(c, y, uv)
    assert uvo[0, 2:, 2:].reshape(-1, 2).tolist() == [[(403 + 2) // 4, (403 + 2) // 4]] * 4 == [[101, 101]] * 4
    assert np.array_equal(yo, y) and np.array_equal(uvo[0, :2], uv[0, :2]) and m.sum() == 9


# ------------------------------------------------------------------ the palette helper
def test_palette_helper_inverts_the_conversion():
    """rgb_to_yuv then the NV12 block's integer conversion gives back the colour within the two
    roundings, for both matrices and both ranges; the anchors are exact. The bound: half a level of Y
    times cy / 256 <= 1.17, half a level of chroma times the largest coefficient 541 / 256 = 2.12, the
    conversion's own rounding 0.5 and the table's: below 2.4, so at most 3 levels."""
    import test_nv12_host as NH
    rgb = np.array(A.DEFAULT_PALETTE + ((0, 0, 0), (255, 255, 255), (128, 128, 128)), np.uint8)
    for (matrix, rng), coef in sorted(NH.N.COEF.items()):
        yuv = A.rgb_to_yuv(rgb, matrix, rng)
        back = np.stack([NH.nv12_to_rgb_ref(p[:1].reshape(1, 1, 1), p[1:].reshape(1, 1, 1, 2), coef)[0, 0, 0] for p in yuv])
        assert np.abs(back.astype(int) - rgb.astype(int)).max() <= 3, (matrix, rng)
        lo, hi = (16, 235) if rng == "limited" else (0, 255)
        assert yuv[-3].tolist() == [lo, 128, 128] and yuv[-2].tolist() == [hi, 128, 128]
    assert A.rgb_to_yuv([(255, 0, 0)], "bt601", "full").tolist() == [[76, 85, 255]]
    assert A.rgb_to_yuv([(255, 0, 0)], "bt709", "limited").tolist() == [[63, 102, 240]]
    with pytest.raises(ValueError):
        A.rgb_to_yuv([(1, 2, 3)], "bt2020")


# ------------------------------------------------------------------ the ABI and the refusals
NEW = {"prpe_annotate_geometry": 1, "prpe_annotate_table_bytes": 4, "prpe_annotate_nv12": 3, "prpe_annotate_u8": 3}


def test_abi_table_has_the_annotate_entry_points():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name, nargs in NEW.items():
        decl = re.search(r"\b(?:int|int64_t|void) " + name + r"\s*\(([^;]*)\);", bare)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    body = re.search(r"typedef struct prpe_annotate_args \{(.*?)\} prpe_annotate_args;", bare, re.S).group(1)
    names = [re.sub(r"[\s*]", "", v).split(" ")[-1] for d in body.split(";") if d.strip()
             for v in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", d.strip()).split(",")]
    assert names == [n for n, _ in _lib.AnnotateArgs._fields_]
    # 12 pointers, one int64, 9 int32 and 3 floats
    assert C.sizeof(_lib.AnnotateArgs) == 12 * 8 + 8 + 12 * 4 and _lib.AnnotateArgs.table_bytes.offset == 96
    assert L.prpe_abi_version() == 12 == _lib.ABI_VERSION
    th, tw, sh, sw = ops.annotate_geometry()
    assert sh % th == 0 and sw % tw == 0 and th % 2 == 0 and tw % 8 == 0
    assert ops.annotate_table_bytes(0, 0, 1, 0) == 0
    assert ops.annotate_table_bytes(5, 3, 17, 19) == 4 * (9 * 8 + 5 * 37 * 4)
    for bad in ((-1, 0, 1, 0), (0, 2 ** 20 + 1, 1, 0), (1, 1, 0, 0), (1, 1, 65, 0), (1, 1, 17, 33), (1, 1, 17, -1)):
        assert L.prpe_annotate_table_bytes(*bad) == -22


P0 = 0x10000


def lib_args(**kw):
    """prpe_annotate_args that the library takes, on addresses it never dereferences before a launch."""
    limbs = kw.pop("limbs_list", [0, 1, 1, 2])
    v = dict(crop_meta_p=P0, n_p=P0, keypoints=P0, person_colour=P0, crop_meta_f=P0, n_f=P0, face_mode=P0, face_colour=P0,
             palette=P0, limbs=(C.c_int32 * max(len(limbs), 1))(*limbs), table=P0, means=P0, table_bytes=1 << 20,
             max_p=4, K=17, max_f=3, n_colours=5, n_limbs=len(limbs) // 2, box_t=2, limb_r=1, kp_r=2, cell=8, kp_thr=0.3,
             sx=1.0, sy=1.0)
    v.update(kw)
    if v["limbs"] is None:
        v["limbs"] = C.POINTER(C.c_int32)()
    return _lib.AnnotateArgs(**v)


def lib_refusals():
    """name -> keyword changes of ``lib_args``: every -EINVAL cause of the header that is not the surface's."""
    r = {f"null {k}": {k: None} for k in ("crop_meta_p", "n_p", "keypoints", "person_colour", "crop_meta_f", "n_f",
                                          "face_mode", "face_colour", "palette", "limbs", "table", "means")}
    r.update({"K 0": dict(K=0), "K 65": dict(K=65), "limbs 33": dict(limbs_list=[0, 1] * 33), "limb index K": dict(limbs_list=[0, 17]),
              "limb index -1": dict(limbs_list=[-1, 2]), "max_p -1": dict(max_p=-1), "max_f big": dict(max_f=2 ** 20 + 1),
              "box_t 17": dict(box_t=17), "box_t -1": dict(box_t=-1), "limb_r 17": dict(limb_r=17), "limb_r -1": dict(limb_r=-1),
              "kp_r 17": dict(kp_r=17), "kp_r -1": dict(kp_r=-1), "cell odd": dict(cell=7), "cell 0": dict(cell=0),
              "cell 66": dict(cell=66), "no colours": dict(n_colours=0), "sx 0": dict(sx=0.0), "sx -1": dict(sx=-1.0),
              "sx nan": dict(sx=NAN), "sy inf": dict(sy=INF), "sy 0": dict(sy=0.0), "kp_thr nan": dict(kp_thr=NAN),
              "palette odd": dict(palette=P0 + 2), "means odd": dict(means=P0 + 2), "table 8": dict(table=P0 + 8),
              "table small": dict(table_bytes=ops.annotate_table_bytes(4, 3, 17, 2) - 1)})
    return r


NV_GOOD = dict(y=P0, uv=P0 + 0x4000, n=2, h=9, w=13, y_sn=1024, y_sh=16, uv_sn=512, uv_sh=14)
NV_BAD = [dict(y=None), dict(uv=None), dict(n=0), dict(h=0), dict(w=0), dict(h=16385), dict(w=16385, y_sh=2 ** 15, uv_sh=2 ** 15),
          dict(y_sh=12), dict(uv_sh=12), dict(uv=P0 + 0x4001), dict(uv_sn=511), dict(uv_sh=15)]
U8_GOOD = dict(ptr=P0, n=2, h=9, w=13, c=3, sn=1024, sh=64, sw=3, sc=1)
U8_BAD = [dict(ptr=None), dict(n=0), dict(h=0), dict(w=0), dict(c=4), dict(c=1), dict(h=16385), dict(w=16385)]


def nv_surface(**kw):
    v = dict(NV_GOOD, **kw)
    return _lib.NV12(v["y"], v["uv"], v["n"], v["h"], v["w"], v["y_sn"], v["y_sh"], v["uv_sn"], v["uv_sh"])


def u8_surface(**kw):
    v = dict(U8_GOOD, **kw)
    return _lib.View(v["ptr"], v["n"], v["h"], v["w"], v["c"], v["sn"], v["sh"], v["sw"], v["sc"])


def test_library_refuses_bad_annotate_arguments_before_launch():
    L = _lib.lib()
    for name, call, good, bads in (("nv12", L.prpe_annotate_nv12, nv_surface, NV_BAD),
                                   ("u8", L.prpe_annotate_u8, u8_surface, U8_BAD)):
        assert call(None, C.byref(lib_args()), None) == -22 and call(C.byref(good()), None, None) == -22
        for kw in bads:
            assert call(C.byref(good(**kw)), C.byref(lib_args()), None) == -22, (name, kw)
        for cause, kw in sorted(lib_refusals().items()):
            assert call(C.byref(good()), C.byref(lib_args(**kw)), None) == -22, (name, cause)
        # nothing to draw from: legal, and nothing is launched or dereferenced
        assert call(C.byref(good()), C.byref(lib_args(max_p=0, max_f=0, table=None, means=None, crop_meta_p=None,
                                                      n_p=None, crop_meta_f=None)), None) == 0


def test_wrappers_and_annotator_check_before_the_library():
    y, uv, img = (torch.from_numpy(a) for a in surfaces(1, 8, 10, 0))
    pal = torch.zeros(3, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="HIP device"):
        ops.annotate_u8(img, pal)
    with pytest.raises(ValueError, match="device"):
        ops.annotate_nv12(NV12Frames(y, uv), pal)
    with pytest.raises(ValueError, match="NV12Frames"):
        ops.annotate_nv12(img, pal)
    for kw in (dict(colour_by="name"), dict(redact="some"), dict(redact_mode="blur"), dict(channel_order="gbr"),
               dict(palette_rgb=[(1, 2)]), dict(palette_rgb=[(1, 2, 300)])):
        with pytest.raises(ValueError):
            Annotator(**kw)
    a = Annotator(redact="unknown")
    with pytest.raises(ValueError, match="mixed sizes"):
        a([img, img], {})
    with pytest.raises(ValueError, match="track_id"):
        a(img, {"crop_meta": torch.zeros(2, 8), "n_crops": torch.zeros(1, dtype=torch.int32),
                "keypoints": torch.zeros(2, 17, 3)})
    with pytest.raises(ValueError, match="faces"):
        Annotator(colour_by="slot", redact="all")(img, {"crop_meta": torch.zeros(2, 8),
                                                        "n_crops": torch.zeros(1, dtype=torch.int32),
                                                        "keypoints": torch.zeros(2, 17, 3)})
    # the lists on the host: torch ops only
    out = {"pose": {"crop_meta": torch.zeros(3, 8), "n_crops": torch.tensor([3], dtype=torch.int32),
                    "keypoints": torch.zeros(3, 17, 3)},
           "faces": {"crop_meta": torch.zeros(4, 8), "n_crops": torch.tensor([4], dtype=torch.int32),
                     "ident": torch.tensor([5, -1, 0, -1])},
           "track_id": torch.tensor([14, -1, 3], dtype=torch.int32), "person_ident": torch.tensor([-1, 7, 25])}
    persons, faces = a.lists(out)
    assert persons[3].tolist() == [2, 12, 3] and persons[3].dtype == torch.int32
    assert faces[2].tolist() == [0, 1, 0, 1] and faces[3].tolist() == [13] * 4
    assert Annotator(colour_by="ident", redact="known", redact_mode="fill").lists(out)[1][2].tolist() == [2, 0, 2, 0]
    assert Annotator(colour_by="ident").lists(out)[0][3].tolist() == [12, 7, 1]
    assert Annotator(colour_by="slot", redact="all").lists(out)[1][2].tolist() == [1] * 4
    assert Annotator(colour_by="slot").lists(out["pose"])[0][3].tolist() == [0, 1, 2]
    assert len(ops.COCO_LIMBS) == 19 and {v for ab in ops.COCO_LIMBS for v in ab} == set(range(17))
