"""CPU: face crops aligned to the skeleton's eyes and nose (csrc/facealign.hip, prpe.faces; DESIGN.md
§5h) as far as the host goes -- ``face_align_fit_ref``, a plain fp64 restatement of the fit and its
gates, held to numpy's least squares on the 6-equation system and to hand cases; ``roi_warp_ref``, a
plain restatement of the resampling, held to F.grid_sample; the ABI table and the refusals; the host
helpers. tests/test_gpu_facealign.py holds the kernels to the two restatements."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import test_faces_host as FH
from prpe import _lib
from prpe.ops import WARP_COLS                     # the warp row's columns: flag, person slot, a, b, tx, c, d, ty

NAN, INF = float("nan"), float("inf")
f32 = np.float32
# the ArcFace positions in a 112 x 112 crop: the eye on the viewer's left, the eye on the viewer's
# right, the nose; paired with COCO keypoints 2 (right eye), 1 (left eye), 0 (nose)
TEMPLATE = ((38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366))
TEMPLATE_KP = (2, 1, 0)


def template(out_hw):
    """The template points of an out_h x out_w crop, as include/prpe.h forms them."""
    kx, ky = out_hw[1] / 112.0, out_hw[0] / 112.0
    return [(x * kx, y * ky) for x, y in TEMPLATE]


def similarity_fit(q, p):
    """include/prpe.h's closed form on python floats (fp64, one rounding per operation, sums in
    ascending order from 0): (A, C, TX, TY) of x = A qx - C qy + TX, y = C qx + A qy + TY."""
    qmx, qmy = (q[0][0] + q[1][0] + q[2][0]) / 3.0, (q[0][1] + q[1][1] + q[2][1]) / 3.0
    pmx, pmy = (p[0][0] + p[1][0] + p[2][0]) / 3.0, (p[0][1] + p[1][1] + p[2][1]) / 3.0
    D = dot = cross = 0.0
    for (qx, qy), (px, py) in zip(q, p):
        ux, uy, vx, vy = qx - qmx, qy - qmy, px - pmx, py - pmy
        D = D + (ux * ux + uy * uy)
        dot = dot + (ux * vx + uy * vy)
        cross = cross + (ux * vy - uy * vx)
    A, Cc = dot / D, cross / D
    return A, Cc, pmx - (A * qmx - Cc * qmy), pmy - (Cc * qmx + A * qmy)


def similarity_lstsq(q, p):
    """The independent statement: numpy's least squares on the six equations in (A, C, TX, TY)."""
    rows, rhs = [], []
    for (qx, qy), (px, py) in zip(q, p):
        rows += [[qx, -qy, 1.0, 0.0], [qy, qx, 0.0, 1.0]]
        rhs += [px, py]
    sol, *_ = np.linalg.lstsq(np.array(rows, np.float64), np.array(rhs, np.float64), rcond=None)
    return tuple(float(v) for v in sol)


def face_align_fit_ref(meta_f, n_f, n_p, kpts, person_face, out_hw, kp_thr=0.3, scale=(0.5, 2.0)):
    """prpe_face_align_fit on the host: warp [F, 8] float32 (torch), zero where no row is written."""
    meta, kp, pf = meta_f.numpy(), kpts.numpy().astype(f32), person_face.numpy()
    Fn, P = meta.shape[0], kp.shape[0]
    warp = np.zeros((Fn, WARP_COLS), f32)
    n_p, n_f = min(int(n_p), P), min(int(n_f), Fn)
    oh, ow = out_hw
    q = template(out_hw)
    lo, hi, thr = float(f32(scale[0])), float(f32(scale[1])), f32(kp_thr)
    with np.errstate(all="ignore"):
        for s in range(max(n_p, 0)):
            fs = int(pf[s])
            if fs < 0 or fs >= n_f:
                continue
            pts = [kp[s, k] for k in TEMPLATE_KP]
            if not all(pt[2] >= thr and np.isfinite(pt[0]) and np.isfinite(pt[1]) for pt in pts):
                continue
            A, Cc, TX, TY = similarity_fit(q, [(float(pt[0]), float(pt[1])) for pt in pts])
            a, c, tx, ty = f32(A), f32(Cc), f32(TX), f32(TY)
            b, d = f32(-Cc), a
            if not all(np.isfinite(v) for v in (a, c, tx, ty)):
                continue
            x0, y0, w, h = (f32(v) for v in meta[fs, 2:6])
            size = f32(math.sqrt(float(a) * float(a) + float(c) * float(c)) * float(ow))
            if not (lo * float(w) <= float(size) <= hi * float(w)):
                continue
            u, v = 0.5 * ow, 0.5 * oh
            cx = f32((float(a) * u + float(b) * v) + float(tx))
            cy = f32((float(c) * u + float(d) * v) + float(ty))
            if not (cx >= x0 and cx <= x0 + w and cy >= y0 and cy <= y0 + h):      # fp32 sums
                continue
            warp[fs] = (0.0, 0.0, a, b, tx, c, d, ty)
            warp.view(np.int32)[fs, :2] = (1, s)
    return torch.from_numpy(warp)


def warp_theta(coef, out_hw, frame_hw):
    """F.affine_grid's theta [1, 2, 3] (fp64, align_corners=False) of the map (a, b, tx, c, d, ty)."""
    a, b, tx, c, d, ty = (float(v) for v in coef)
    (oh, ow), (H, W) = out_hw, frame_hw
    return torch.tensor([[[a * ow / W, b * oh / W, (a * ow + b * oh + 2 * tx) / W - 1.0],
                          [c * ow / H, d * oh / H, (c * ow + d * oh + 2 * ty) / H - 1.0]]], dtype=torch.float64)


def warp_yardstick(frames64, f, coef, out_hw, round_grid=False):
    """F.affine_grid + F.grid_sample(bilinear, zeros, align_corners=False) in float64 -> [3, oh, ow];
    ``round_grid``: the same with its grid rounded to fp32 (the yardstick's own fp32 noise)."""
    grid = F.affine_grid(warp_theta(coef, out_hw, frames64.shape[2:]), (1, 3, out_hw[0], out_hw[1]), align_corners=False)
    if round_grid:
        grid = grid.float().double()
    return F.grid_sample(frames64[f:f + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]


def roi_warp_ref(frames, f, coef, out_hw):
    """prpe_roi_warp's flagged path on the host: frames [B, 3, H, W] float32 (torch), ``coef`` =
    (a, b, tx, c, d, ty) fp32 -> [3, oh, ow] float32. Coordinates in fp64, clamped to [-2, size + 1]
    (NaN -> -2), one fp32 rounding per weight, fp32 lerps, taps outside the frame 0."""
    img = frames[f].numpy().astype(f32)
    H, W = img.shape[1:]
    oh, ow = out_hw
    a, b, tx, c, d, ty = (float(f32(v)) for v in coef)
    with np.errstate(all="ignore"):
        j, i = np.arange(ow) + 0.5, np.arange(oh) + 0.5
        sx = (a * j + tx)[None, :] + (b * i)[:, None] - 0.5
        sy = (c * j + ty)[None, :] + (d * i)[:, None] - 0.5

        def taps(s, size):
            s = np.fmin(np.fmax(s, -2.0), size + 1.0)                 # fmax / fmin drop a NaN
            fl = np.floor(s)
            return (s - fl).astype(f32), fl.astype(np.int64)
        ax, ix = taps(sx, W)
        ay, iy = taps(sy, H)

        def at(yy, xx):
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            return np.where(ok[None], img[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], f32(0))
        v00, v01, v10, v11 = at(iy, ix), at(iy, ix + 1), at(iy + 1, ix), at(iy + 1, ix + 1)
        top = v00 + ax[None] * (v01 - v00)
        bot = v10 + ax[None] * (v11 - v10)
        out = top + ay[None] * (bot - top)
    assert out.dtype == f32
    return torch.from_numpy(out)


def window_coef(win, out_hw):
    """The map that samples exactly the window (x0, y0, w, h)."""
    x0, y0, w, h = win
    return (w / out_hw[1], 0.0, x0, 0.0, h / out_hw[0], y0)


def roll_coef(deg, size, centre, out_hw):
    """A crop ``size`` frame pixels wide about ``centre``, rolled by ``deg``."""
    s = size / out_hw[1]
    a, c = s * math.cos(math.radians(deg)), s * math.sin(math.radians(deg))
    u, v = 0.5 * out_hw[1], 0.5 * out_hw[0]
    return (a, -c, centre[0] - (a * u - c * v), c, a, centre[1] - (c * u + a * v))


# ---------------------------------------------------------------------------------- the fit
def test_closed_form_agrees_with_lstsq_on_random_triples():
    rng = np.random.default_rng(11)
    worst = 0.0
    for out_hw in ((112, 112), (8, 12), (9, 130)):
        q = template(out_hw)
        for _ in range(200):
            p = [tuple(v) for v in rng.uniform(-50.0, 700.0, (3, 2))]
            got, want = similarity_fit(q, p), similarity_lstsq(q, p)
            scale = max(1.0, max(abs(v) for v in want))
            worst = max(worst, max(abs(g - w) for g, w in zip(got, want)) / scale)
    print(f"closed form against lstsq: largest relative difference {worst:.3e}")
    assert worst <= 1e-12


def _apply(fit, pt):
    A, Cc, TX, TY = fit
    return A * pt[0] - Cc * pt[1] + TX, Cc * pt[0] + A * pt[1] + TY


def test_fit_hand_cases():
    q = template((112, 112))
    # the face exactly on the template: the identity
    A, Cc, TX, TY = similarity_fit(q, q)
    assert abs(A - 1) < 1e-14 and abs(Cc) < 1e-14 and abs(TX) < 1e-12 and abs(TY) < 1e-12
    # the template of a 56 x 56 crop placed 3x larger at (100, 40): scale 3, offset (100, 40)
    q2 = template((56, 56))
    A, Cc, TX, TY = similarity_fit(q2, [(100 + 3 * x, 40 + 3 * y) for x, y in q2])
    assert abs(A - 3) < 1e-13 and abs(Cc) < 1e-13 and abs(TX - 100) < 1e-11 and abs(TY - 40) < 1e-11
    # a 90 degree roll (x, y) -> (-y, x) about the origin, then a shift: A = 0, C = 1
    fit = similarity_fit(q, [(200 - y, 50 + x) for x, y in q])
    assert abs(fit[0]) < 1e-14 and abs(fit[1] - 1) < 1e-14 and abs(fit[2] - 200) < 1e-11 and abs(fit[3] - 50) < 1e-11
    # a mirrored face (x -> 112 - x): no similarity without reflection fits it. The fit must stay a
    # rotation-and-scale (d = a, b = -c by construction: determinant a^2 + c^2 >= 0), and must not
    # reproduce the points as the reflection would
    mirrored = [(112 - x, y) for x, y in q]
    fit = similarity_fit(q, mirrored)
    assert fit[0] * fit[0] + fit[1] * fit[1] >= 0.0
    resid = max(math.hypot(gx - mx, gy - my) for (gx, gy), (mx, my) in zip((_apply(fit, pt) for pt in q), mirrored))
    assert resid > 5.0
    want = similarity_lstsq(q, mirrored)
    assert max(abs(g - w) for g, w in zip(fit, want)) < 1e-10


def _one_face(kp_pts, win=(20.0, 10.0, 40.0, 40.0), scores=(0.9, 0.9, 0.9), K=17):
    """One person (slot 0) with nose, left eye, right eye = kp_pts (COCO order) matched to one face."""
    meta = torch.zeros(2, 8)
    meta.view(torch.int32)[:, 0] = torch.tensor([0, -1])
    meta[0, 2:6] = torch.tensor(win)
    kp = torch.zeros(2, K, 3)
    for k, (pt, sc) in enumerate(zip(kp_pts, scores)):
        kp[0, k] = torch.tensor([pt[0], pt[1], sc])
    return meta, 1, 1, kp, torch.tensor([0, -1], dtype=torch.int32)


def _coco(points):
    """template order (right eye, left eye, nose) -> COCO order (nose, left eye, right eye)."""
    return [points[2], points[1], points[0]]


def test_fit_ref_writes_the_row_and_applies_each_gate():
    out_hw = (112, 112)
    # the template, 0.375 x, at (22, 12): a crop 42 pixels wide about (43, 33), window 40 x 40 about (40, 30)
    pts = [(22 + 0.375 * x, 12 + 0.375 * y) for x, y in template(out_hw)]
    args = _one_face(_coco(pts))
    warp = face_align_fit_ref(*args, out_hw)
    assert warp.view(torch.int32)[0, :2].tolist() == [1, 0] and float(warp[1].abs().max()) == 0.0
    a, b, tx, c, d, ty = (float(v) for v in warp[0, 2:])
    assert abs(a - 0.375) < 1e-6 and a == d and b == -c and abs(c) < 1e-6 and abs(tx - 22) < 1e-4 and abs(ty - 12) < 1e-4
    zero = lambda **kw: float(face_align_fit_ref(*args, out_hw, **kw).abs().max()) == 0.0
    assert zero(kp_thr=0.95)                           # a keypoint below the threshold
    assert not zero(kp_thr=0.9)                        # at the threshold: kept
    assert zero(scale=(1.1, 2.0)) and zero(scale=(0.5, 1.0)) and not zero(scale=(1.0, 1.1))       # 42 / 40
    # both ends are inclusive: over a 32-pixel window the ratio size / 32 is an fp32 number
    wide = _one_face(_coco(pts), win=(27.0, 17.0, 32.0, 32.0))
    size = f32(math.sqrt(a * a + c * c) * 112.0)
    r = f32(float(size) / 32.0)
    up, down = float(np.nextafter(r, f32(INF))), float(np.nextafter(r, f32(-INF)))
    some = lambda lo, hi: float(face_align_fit_ref(*wide, out_hw, scale=(lo, hi)).abs().max()) > 0.0
    assert float(r) * 32.0 == float(size) and some(float(r), float(r))
    assert not some(up, 2.0) and not some(0.5, down) and some(down, up)
    for bad in (NAN, INF):
        moved = [list(p) for p in _coco(pts)]
        moved[1][0] = bad
        assert float(face_align_fit_ref(*_one_face(moved), out_hw).abs().max()) == 0.0
    assert float(face_align_fit_ref(*_one_face(_coco(pts), win=(70.0, 10.0, 40.0, 40.0)), out_hw).abs().max()) == 0.0
    # eyes that coincide (a profile): the crop collapses, the scale gate refuses it
    flat = _coco([(40.0, 30.0), (40.0, 30.0), (40.0, 31.0)])
    assert float(face_align_fit_ref(*_one_face(flat), out_hw).abs().max()) == 0.0
    # person_face -1, >= n_f, a slot past n_p
    meta, n_f, n_p, kp, pf = args
    assert float(face_align_fit_ref(meta, n_f, n_p, kp, torch.tensor([-1, -1], dtype=torch.int32), out_hw).abs().max()) == 0
    assert float(face_align_fit_ref(meta, n_f, n_p, kp, torch.tensor([1, -1], dtype=torch.int32), out_hw).abs().max()) == 0
    assert float(face_align_fit_ref(meta, n_f, 0, kp, pf, out_hw).abs().max()) == 0


# ---------------------------------------------------------------------------------- the resampling
def test_roi_warp_ref_against_grid_sample_and_the_window_route():
    g = torch.Generator().manual_seed(3)
    fr = torch.rand(2, 3, 40, 56, generator=g)
    out_hw = (9, 13)
    for coef in (roll_coef(0, 20.0, (28.0, 20.0), out_hw), roll_coef(30, 20.0, (28.0, 20.0), out_hw),
                 roll_coef(90, 30.0, (10.0, 8.0), out_hw), roll_coef(180, 70.0, (28.0, 20.0), out_hw)):
        coef = tuple(float(f32(v)) for v in coef)
        exact = warp_yardstick(fr.double(), 1, coef, out_hw)
        noise = float((warp_yardstick(fr.double(), 1, coef, out_hw, True) - exact).abs().max())
        err = float((roi_warp_ref(fr, 1, coef, out_hw).double() - exact).abs().max())
        assert 0.0 < noise < 1e-4 and err <= 4 * noise and float(exact.abs().max()) > 0.2
    # the map of a window is the window's resample (tests/test_faces_host.py's yardstick)
    win = (12.5, 6.0, 26.0, 18.0)
    coef = tuple(float(f32(v)) for v in window_coef(win, out_hw))
    want = FH.roi_resize_ref(fr.double(), 0, win, out_hw)
    assert float((roi_warp_ref(fr, 0, coef, out_hw).double() - want).abs().max()) < 1e-5
    # the identity map returns the frame; wild coefficients are all taps outside: zeros
    assert torch.equal(roi_warp_ref(fr, 0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (40, 56)), fr[0])
    for wild in ((1e30, 0.0, 0.0, 0.0, 1.0, 0.0), (NAN, 0.0, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, INF, 0.0, 1.0, -INF),
                 (1.0, 0.0, 500.0, 0.0, 1.0, 0.0)):
        assert float(roi_warp_ref(fr, 0, wild, out_hw).abs().max()) == 0.0


# ---------------------------------------------------------------------------------- ABI
ENTRY_POINTS = (("prpe_face_align_fit", 15), ("prpe_roi_warp", 8), ("prpe_roi_warp_u8", 11))


def test_abi_table_has_the_align_entry_points_and_the_abi_is_still_12():
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


def test_library_rejects_bad_align_arguments_before_launch():
    L = _lib.lib()
    p = 0x1000

    def fit(meta=p, n_f=p, max_f=4, n_p=p, max_p=4, kp=p, K=17, pf=p, oh=112, ow=112, thr=0.3, lo=0.5, hi=2.0, warp=p):
        return L.prpe_face_align_fit(meta, n_f, max_f, n_p, max_p, kp, K, pf, oh, ow, thr, lo, hi, warp, None)
    for name in ("meta", "n_f", "n_p", "kp", "pf", "warp"):
        assert fit(**{name: None}) == -22, name
    assert fit(max_f=0) == -22 and fit(max_p=0) == -22 and fit(K=2) == -22 and fit(thr=NAN) == -22
    for bad in (0, -1, 4097):
        assert fit(oh=bad) == -22 and fit(ow=bad) == -22
    assert fit(lo=0.0) == -22 and fit(lo=-1.0) == -22 and fit(lo=NAN) == -22 and fit(hi=NAN) == -22
    assert fit(lo=2.5) == -22                          # above scale_hi

    fr = _lib.View(p, 1, 8, 8, 3, 192, 24, 3, 1)
    fr4 = _lib.View(p, 1, 8, 8, 4, 256, 32, 4, 1)
    a3 = (C.c_float * 3)(1.0, 1.0, 1.0)

    def y(ptr=p, n=2, h=12, w=12, c=4, sn=12 * 16 * 4, sh=16 * 4, sw=4, sc=1):
        return _lib.View(ptr, n, h, w, c, sn, sh, sw, sc)

    def both(frames=fr, meta=p, n_crops=p, max_crops=2, warp=p, yv=None):
        yv = y() if yv is None else yv
        r1 = L.prpe_roi_warp(C.byref(frames), meta, n_crops, max_crops, warp, C.byref(yv), None, None)
        r2 = L.prpe_roi_warp_u8(C.byref(frames), meta, n_crops, max_crops, warp, a3, a3, 0, C.byref(yv), None, None)
        assert r1 == r2
        return r1
    assert both(warp=None) == -22
    assert both(frames=fr4) == -22 and both(meta=None) == -22 and both(n_crops=None) == -22
    assert both(max_crops=0) == -22 and both(max_crops=3) == -22
    assert both(yv=y(ptr=None)) == -22 and both(yv=y(sc=2)) == -22 and both(yv=y(ptr=p + 4)) == -22
    assert both(yv=y(sw=6)) == -22 and both(yv=y(sh=66)) == -22 and both(yv=y(c=3)) == -22
    assert both(yv=y(h=4097)) == -22 and both(yv=y(w=4097)) == -22
    assert L.prpe_roi_warp(None, p, p, 2, p, C.byref(y()), None, None) == -22
    assert L.prpe_roi_warp_u8(C.byref(fr), p, p, 2, p, None, a3, 0, C.byref(y()), None, None) == -22
    assert L.prpe_roi_warp_u8(C.byref(fr), p, p, 2, p, a3, None, 0, C.byref(y()), None, None) == -22


# ---------------------------------------------------------------------------------- host helpers
def test_ops_validate_arguments_before_any_launch():
    from prpe import ops
    for name in ("face_align_fit", "roi_warp", "roi_warp_u8"):
        assert callable(getattr(ops, name))
    assert ops.WARP_COLS == 8
    meta, n = torch.zeros(4, 8), torch.zeros(1, dtype=torch.int32)
    kp, pf, warp = torch.zeros(3, 17, 3), torch.zeros(3, dtype=torch.int32), torch.zeros(4, 8)
    with pytest.raises(ValueError, match="crop_meta_f"):
        ops.face_align_fit(torch.zeros(8), n, n, kp, pf, (112, 112), warp=warp)
    with pytest.raises(ValueError, match="keypoints"):
        ops.face_align_fit(meta, n, n, torch.zeros(3, 17, 2), pf, (112, 112), warp=warp)
    with pytest.raises(ValueError, match="crop_meta_f"):
        ops.face_align_fit(meta, n, n, kp, pf, (112, 112), warp=warp)                  # host tensors
    with pytest.raises(ValueError, match="frames"):
        ops.roi_warp(torch.zeros(1, 3, 8, 8), meta, n, warp, torch.zeros(4, 12, 12, 4))
    with pytest.raises(ValueError, match="frames"):
        ops.roi_warp_u8(torch.zeros(1, 8, 8, 3), meta, n, warp, torch.zeros(4, 12, 12, 4))          # not uint8


def test_person_recognition_align_arguments():
    from prpe import FaceGallery, PersonRecognition
    model = object()                                  # the constructor does not touch the model
    g = FaceGallery(dim=512, capacity=2, device="cpu")
    pr = PersonRecognition(model, g)
    assert pr.align is False and pr.align_scale == (0.5, 2.0)
    pr = PersonRecognition(model, g, align=True, align_scale=(0.75, 1.5))
    assert pr.align is True and pr.align_scale == (0.75, 1.5)
    for bad in ((0.0, 2.0), (2.0, 1.0), (NAN, 2.0), (0.5, NAN)):
        with pytest.raises(ValueError, match="align_scale"):
            PersonRecognition(model, g, align=True, align_scale=bad)
    for name in ("from_pose", "from_pose_u8", "enrol", "enrol_u8", "enrol_pose"):
        assert callable(getattr(pr, name))


def test_results_report_which_faces_were_aligned():
    from prpe import PersonRecognition
    import test_topdown_host as T
    out_f = FH._face_out([[((10, 20, 30, 40), 0.9, 7, 0.75), ((50, 50, 70, 70), 0.7, 3, 0.5)]], 3)
    d, c = T._dets([[(10, 20, 50, 120, 0.9), (0, 0, 120, 40, 0.8), (8, 16, 200, 272, 0.7)]])
    meta, n, st = T.select_ref(d, c, max_crops=4)
    out_p = {"dets": d, "counts": c, "crop_meta": meta, "n_crops": torch.tensor([n], dtype=torch.int32),
             "status": torch.tensor([st], dtype=torch.int32), "keypoints": torch.zeros(4, 17, 3)}
    out = {"pose": out_p, "faces": out_f, "person_face": torch.tensor([1, -1, 0, -1], dtype=torch.int32),
           "person_ident": torch.tensor([3, -1, 7, -1]), "person_score": torch.tensor([0.5, -INF, 0.75, -INF]),
           "match_status": torch.zeros(1, dtype=torch.int32)}
    assert [p["face_aligned"] for p in PersonRecognition.results(out)[0]] == [False, False, False]
    warp = torch.zeros(3, 8)
    warp.view(torch.int32)[1, :2] = torch.tensor([1, 0])          # face slot 1, from person slot 0
    people = PersonRecognition.results(dict(out, face_warp=warp))[0]
    assert [p["face_aligned"] for p in people] == [True, False, False]
    assert [p["ident"] for p in people] == [3, -1, 7] and people[2]["face_box"] == [7.5, 17.5, 32.5, 42.5]
