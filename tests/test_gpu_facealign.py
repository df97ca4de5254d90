"""GPU: face crops aligned to the skeleton's eyes and nose (csrc/facealign.hip, prpe.faces; DESIGN.md
§5h) -- the kernels against the restatements of tests/test_facealign_host.py, against
prpe_roi_resize where no row is flagged, and PersonRecognition(align=True) against the unfused route
through the public ops.

Tolerances (none is taken from what the kernels give):
* face_align_fit: flag and person columns bit-equal to ``face_align_fit_ref``; each coefficient within
  2^-23 max(|v|, 1) of the fp64 statement rounded to fp32 (the closed form and lstsq differ near
  1e-13, far below half an fp32 ulp, so only the final rounding can differ).
* roi_warp, unflagged rows: every bit of prpe_roi_resize / prpe_roi_resize_u8, y_amax included.
* roi_warp, flagged rows: the yardstick is F.affine_grid + F.grid_sample(bilinear, zeros,
  align_corners=False) in float64 on the CPU with theta from the fp32 warp rows read back; its own
  fp32 noise e = max |yardstick - yardstick with its grid rounded to fp32| over the launch's warps;
  the kernel is allowed 4 e (tests/test_gpu_faces.py's and DESIGN.md §5b's convention).
* PersonRecognition(align=True): bit-identical to the unfused route; enrolled crops score within
  4 x the fp32 CPU normalise-and-dot's own distance from fp64 of 1.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_facealign_host as AH
import test_faces_host as FH
import test_gpu_faces as GF
from prpe import CombinedModel, FaceGallery, FrameIngest, PersonRecognition, TopDownPose, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
H, W = GF.H, GF.W
f32 = np.float32
_bits, _same = GF._bits, GF._same


def _up(v):
    return float(np.nextafter(f32(v), f32(INF)))


def _down(v):
    return float(np.nextafter(f32(v), f32(-INF)))


def _i32(v):
    return torch.tensor([v], device=DEV, dtype=torch.int32)


def _on_template(coef, out_hw):
    """(nose, left eye, right eye) where the map ``coef`` puts the template's points."""
    a, b, tx, c, d, ty = coef
    pts = [(a * x + b * y + tx, c * x + d * y + ty) for x, y in AH.template(out_hw)]
    return [pts[2], pts[1], pts[0]]


# ---------------------------------------------------------------------------------- face_align_fit
def _fit_cases(out_hw):
    """-> (meta_f, n_f, n_p, kpts, person_face, expected flag per face row). Person s is matched to
    face s unless said otherwise; the base face is a crop 42 frame pixels wide about (43, 33), rolled
    by 10 degrees, every gate decided at equality from the restatement's own fp32 size and centre."""
    base = _on_template(AH.roll_coef(10, 42.0, (43.0, 33.0), out_hw), out_hw)
    probe = AH.face_align_fit_ref(*AH._one_face(base, win=(27.0, 17.0, 32.0, 32.0)), out_hw)
    assert int(probe.view(torch.int32)[0, 0]) == 1
    a, b, tx, c, d, ty = (float(v) for v in probe[0, 2:])
    size = float(f32(math.sqrt(a * a + c * c) * out_hw[1]))
    cx = float(f32((a * 0.5 * out_hw[1] + b * 0.5 * out_hw[0]) + tx))
    cy = float(f32((c * 0.5 * out_hw[1] + d * 0.5 * out_hw[0]) + ty))
    assert abs(size - 42) < 1e-3 and abs(cx - 43) < 1e-3 and abs(cy - 33) < 1e-3
    good = (0.9, 0.9, 0.9)
    thr = float(f32(0.3))
    about = lambda w: (43.0 - w / 2, 33.0 - w / 2, w, w)
    rows = [  # (keypoints, scores, face window, expected flag)
        (base, good, (27.0, 17.0, 32.0, 32.0), 1),
        # the scale gate, 0.5 w <= size <= 2 w (exact products): both ends at equality and one fp32 past
        (base, good, about(2 * size), 1), (base, good, about(_up(2 * size)), 0),
        (base, good, about(size / 2), 1), (base, good, about(_down(size / 2)), 0),
        # the centre gate on each side of each axis: x0 <= cx <= x0 + w, y0 <= cy <= y0 + h
        (base, good, (cx, 17.0, 32.0, 32.0), 1), (base, good, (_up(cx), 17.0, 32.0, 32.0), 0),
        (base, good, (cx - 32.0, 17.0, 32.0, 32.0), 1), (base, good, (_down(cx) - 32.0, 17.0, 32.0, 32.0), 0),
        (base, good, (27.0, cy, 32.0, 32.0), 1), (base, good, (27.0, _up(cy), 32.0, 32.0), 0),
        (base, good, (27.0, cy - 32.0, 32.0, 32.0), 1), (base, good, (27.0, _down(cy) - 32.0, 32.0, 32.0), 0),
        # the keypoint threshold: all three at it, then each one an fp32 below
        (base, (thr, thr, thr), about(32.0), 1),
        (base, (_down(thr), 0.9, 0.9), about(32.0), 0), (base, (0.9, _down(thr), 0.9), about(32.0), 0),
        (base, (0.9, 0.9, _down(thr)), about(32.0), 0),
        # NaN / inf coordinates (scores above the threshold), a NaN score
        ([(NAN, base[0][1]), base[1], base[2]], good, about(32.0), 0),
        ([base[0], (base[1][0], INF), base[2]], good, about(32.0), 0),
        ([base[0], base[1], (-INF, base[2][1])], good, about(32.0), 0),
        (base, (0.9, NAN, 0.9), about(32.0), 0),
        # finite keypoints whose fit overflows fp32
        ([(0.0, 3e38), (-3e38, 0.0), (3e38, 0.0)], good, about(32.0), 0),
        # eyes that coincide: the crop collapses
        ([(43.0, 34.0), (43.0, 33.0), (43.0, 33.0)], good, about(32.0), 0),
        # a mirrored face (the eyes swapped): no reflection, the crop comes out upside down or tiny, never mirrored
        ([base[0], base[2], base[1]], good, about(32.0), None),
    ]
    for w in (2 * size, size / 2):
        assert float(f32(w)) == w
    assert float(f32(cx - 32.0) + f32(32.0)) == cx and float(f32(_down(cx) - 32.0) + f32(32.0)) == _down(cx)
    assert float(f32(cy - 32.0) + f32(32.0)) == cy and float(f32(_down(cy) - 32.0) + f32(32.0)) == _down(cy)
    n_rows = len(rows)
    # face rows: n_rows matched ones, then: one whose person has person_face = -1, one nobody points
    # at, one pointed at only by a slot past n_p; then rows at or past n_f
    n_f, Fn = n_rows + 3, n_rows + 5
    n_p, P = n_rows + 3, n_rows + 5
    meta = torch.zeros(Fn, 8)
    meta.view(torch.int32)[:, 0] = 0
    meta[:, 2:6] = torch.tensor(about(32.0))
    kp = torch.zeros(P, 17, 3)
    kp[:, :3] = torch.tensor([[x, y, 0.9] for x, y in base])
    pf = torch.full((P,), -1, dtype=torch.int32)
    for s, (pts, sc, win, _) in enumerate(rows):
        meta[s, 2:6] = torch.tensor(win, dtype=torch.float64).float()
        kp[s, :3] = torch.tensor([[x, y, v] for (x, y), v in zip(pts, sc)], dtype=torch.float64).float()
        pf[s] = s
    pf[n_rows] = -1                                    # a good skeleton without a face
    pf[n_rows + 1] = n_f                               # a face slot at n_f ...
    pf[n_rows + 2] = 10 ** 6                           # ... and far past the list
    pf[n_rows + 3] = n_rows + 2                        # slots past n_p that point at valid rows
    pf[n_rows + 4] = 0
    want = [r[3] for r in rows] + [0, 0, 0, 0, 0]
    return meta, n_f, n_p, kp, pf, want


@pytest.mark.parametrize("out_hw", [(112, 112), (8, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_face_align_fit_equals_the_restatement(out_hw):
    meta, n_f, n_p, kp, pf, want = _fit_cases(out_hw)
    Fn = meta.shape[0]
    ref = AH.face_align_fit_ref(meta, n_f, n_p, kp, pf, out_hw)
    buf = torch.full((Fn + 2, 8), 7.0, device=DEV)     # two sentinel rows beyond F
    buf[:Fn] = 0.0
    got = ops.face_align_fit(meta.to(DEV), _i32(n_f), _i32(n_p), kp.to(DEV), pf.to(DEV), out_hw, warp=buf[:Fn])
    assert got.data_ptr() == buf.data_ptr()
    buf = buf.cpu()
    assert bool((buf[Fn:] == 7.0).all())
    got = buf[:Fn]
    flags = ref.view(torch.int32)[:, 0].tolist()
    assert [f for f, w in zip(flags, want) if w is not None] == [w for w in want if w is not None]
    assert torch.equal(_bits(got[:, :2]), _bits(ref[:, :2]))
    assert float(got[torch.tensor(flags) == 0].abs().max()) == 0.0           # untouched rows stay zero
    err = (got[:, 2:].double() - ref[:, 2:].double()).abs()
    allow = 2.0 ** -23 * ref[:, 2:].double().abs().clamp(min=1.0)
    print(f"face_align_fit {out_hw}: flags {flags}; largest coefficient error / allowance {float((err / allow).max()):.3f}")
    assert bool((err <= allow).all())
    hit = [s for s, f in enumerate(flags) if f == 1]
    assert len(hit) >= 8 and ref.view(torch.int32)[hit, 1].tolist() == hit
    rows = got[hit][:, 2:]
    assert torch.equal(rows[:, 0], rows[:, 4]) and torch.equal(rows[:, 1], -rows[:, 3])       # no reflection: d = a, b = -c
    mirrored = len(want) - 6
    if flags[mirrored]:
        assert float(got[mirrored, 2]) == float(got[mirrored, 6])


def test_face_align_fit_user_scale_and_threshold_reach_the_kernel():
    out_hw = (112, 112)
    meta, n_f, n_p, kp, pf, _ = _fit_cases(out_hw)
    for kw in (dict(scale=(1.0, 1.5)), dict(kp_thr=0.95), dict(kp_thr=-1.0, scale=(0.01, 100.0))):
        ref = AH.face_align_fit_ref(meta, n_f, n_p, kp, pf, out_hw, **kw)
        got = ops.face_align_fit(meta.to(DEV), _i32(n_f), _i32(n_p), kp.to(DEV), pf.to(DEV), out_hw,
                                 warp=torch.zeros(meta.shape[0], 8, device=DEV), **kw).cpu()
        assert torch.equal(_bits(got[:, :2]), _bits(ref[:, :2]))
        assert bool(((got[:, 2:].double() - ref[:, 2:].double()).abs()
                     <= 2.0 ** -23 * ref[:, 2:].double().abs().clamp(min=1.0)).all())
    assert int(ref.view(torch.int32)[:, 0].sum()) > int(AH.face_align_fit_ref(meta, n_f, n_p, kp, pf, out_hw)
                                                        .view(torch.int32)[:, 0].sum())


# ---------------------------------------------------------------------------------- roi_warp
def _nan_framed():
    """GF._frames() inside a NaN surround: a strided view whose neighbours must never be read."""
    big = torch.full((3, 3, 48, 64), NAN)
    big[:, :, 4:4 + H, 5:5 + W] = GF._frames()[:, :, 4:4 + H, 5:5 + W]
    return big


def _u8_nan_free():
    big = torch.full((3, 3, 48, 64), 255, dtype=torch.uint8)
    big[:, :, 4:4 + H, 5:5 + W] = GF._u8_frames()[:, :, 4:4 + H, 5:5 + W]
    return big


def _warp_rows(S, flagged=()):
    """[S, 8]: flag 0 rows hold coefficients that must not be looked at."""
    warp = torch.full((S, 8), NAN)
    warp.view(torch.int32)[:, 0] = 0
    warp.view(torch.int32)[:, 1] = -1
    warp.view(torch.int32)[1::2, 0] = 2                # neither 0 nor 1: still the window
    for s, coef in flagged:
        warp.view(torch.int32)[s, 0] = 1
        warp[s, 2:] = torch.tensor(coef, dtype=torch.float64).float()
    return warp


SIZES = [(112, 112), (8, 12), (9, 130)]               # 9 rows: a row tail of 1; 130 columns: the column loop's second trip


@pytest.mark.parametrize("out_hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_roi_warp_without_flags_has_roi_resize_bits(out_hw):
    oh, ow = out_hw
    good, zero = GF._windows(out_hw)
    rows = good + zero
    S = len(rows) + 2
    meta = GF._meta(rows, S)
    meta.view(torch.int32)[len(rows), 0] = 0           # a stale, valid-looking row past n_crops
    meta[len(rows), 2:6] = torch.tensor([5.0, 5.0, 20.0, 20.0])
    meta, n = meta.to(DEV), _i32(len(rows))
    warp = _warp_rows(S).to(DEV)
    frames = _nan_framed().to(DEV)[:, :, 4:4 + H, 5:5 + W]
    u8 = _u8_nan_free().to(DEV)[:, :, 4:4 + H, 5:5 + W].permute(0, 2, 3, 1)
    assert not frames.is_contiguous() and not u8.is_contiguous()
    ing = FrameIngest(norm="imagenet")

    def run(fn, *args, **kw):
        outer = torch.full((S + 1, oh + 3, ow + 5, 4), 7.0, device=DEV)
        amax = torch.zeros(S, device=DEV)
        amax[1] = 5.0                                  # a slot that already holds more keeps it
        fn(*args, outer[:S, 1:1 + oh, 2:2 + ow, :], y_amax=amax, **kw)
        return outer.cpu(), amax.cpu()
    want, want_amax = run(ops.roi_resize, frames, meta, n)
    got, amax = run(ops.roi_warp, frames, meta, n, warp)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(amax), _bits(want_amax))
    assert not bool(torch.isnan(got).any()) and float(want[0].abs().max()) > 0.2 and float(amax[1]) == 5.0
    inner = torch.zeros_like(got, dtype=torch.bool)
    inner[:S, 1:1 + oh, 2:2 + ow, :] = True
    assert bool((got[~inner] == 7.0).all())
    kw = dict(a=ing.a, b=ing.b, swap_rb=True)
    want, want_amax = run(ops.roi_resize_u8, u8, meta, n, **kw)
    got, amax = run(ops.roi_warp_u8, u8, meta, n, warp, **kw)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(amax), _bits(want_amax))
    assert float(want[0].abs().max()) > 0.5
    got_none = torch.full((S, oh, ow, 4), 7.0, device=DEV)
    ops.roi_warp(frames, meta, n, warp, got_none)      # y_amax is optional
    ref_none = torch.full((S, oh, ow, 4), 7.0, device=DEV)
    ops.roi_resize(frames, meta, n, ref_none)
    assert torch.equal(_bits(got_none.cpu()), _bits(ref_none.cpu()))


def _warps(out_hw):
    """(slot rows [(frame, flag-1 coefficients or None, window)], how many are held to the yardstick)."""
    win = (12.3, 6.4, 30.5, 24.25)
    held = [(0, AH.roll_coef(0, 20.0, (28.0, 20.0), out_hw)), (1, AH.roll_coef(30, 20.0, (28.0, 20.0), out_hw)),
            (0, AH.roll_coef(90, 30.0, (30.0, 18.0), out_hw)), (1, AH.roll_coef(180, 26.0, (20.0, 22.0), out_hw)),
            (1, AH.roll_coef(30, 44.0, (5.0, 35.0), out_hw)),          # partly outside the frame
            (2, AH.roll_coef(-75, 25.0, (28.0, 20.0), out_hw))]         # the constant frame
    rows = [(f, coef, win) for f, coef in held]
    rows += [(0, AH.roll_coef(30, 20.0, (500.0, -400.0), out_hw), win),                # wholly outside: zeros
             (1, (1e30, 0.0, 0.0, 0.0, 1e30, 0.0), win), (0, (NAN,) * 6, win),         # the clamp keeps these defined
             (1, (1.0, 0.0, INF, 0.0, 1.0, -INF), win), (0, (-1e30, 1e30, 3e38, 1e-30, 0.0, NAN), win),
             (0, None, win), (1, None, (-3.5, 2.25, 30.0, 20.0)),                      # unflagged rows in the same launch
             (-1, AH.roll_coef(0, 20.0, (28.0, 20.0), out_hw), win),                   # empty slots, flagged
             (3, AH.roll_coef(0, 20.0, (28.0, 20.0), out_hw), win)]
    return rows, len(held)


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def warped(request):
    out_hw = request.param
    oh, ow = out_hw
    rows, n_held = _warps(out_hw)
    S = len(rows) + 1                                  # one slot past n_crops: flagged, a valid-looking frame
    meta = GF._meta([(f, w) for f, _, w in rows] + [(0, rows[0][2])], S)
    flagged = [(s, c) for s, (_, c, _) in enumerate(rows) if c is not None] + [(S - 1, rows[0][1])]
    warp = _warp_rows(S, flagged)
    n = _i32(len(rows))
    frames = _nan_framed().to(DEV)[:, :, 4:4 + H, 5:5 + W]
    outer = torch.full((S + 1, oh + 3, ow + 5, 4), 7.0, device=DEV)
    amax = torch.zeros(S, device=DEV)
    amax[6] = 0.25                                     # the slot wholly outside must leave this alone
    ops.roi_warp(frames, meta.to(DEV), n, warp.to(DEV), outer[:S, 1:1 + oh, 2:2 + ow, :], y_amax=amax)
    plain = torch.zeros(S, oh, ow, 4, device=DEV)
    ops.roi_resize(frames, meta.to(DEV), n, plain)
    return out_hw, rows, n_held, warp, outer.cpu(), amax.cpu(), plain.cpu()


def test_roi_warp_against_cpu_grid_sample(warped):
    out_hw, rows, n_held, warp, outer, _, _ = warped
    oh, ow = out_hw
    frames64 = GF._frames()[:, :, 4:4 + H, 5:5 + W].double()
    got = outer[:, 1:1 + oh, 2:2 + ow, :3]
    exact = [AH.warp_yardstick(frames64, rows[s][0], warp[s, 2:], out_hw) for s in range(n_held)]
    noise = max(float((AH.warp_yardstick(frames64, rows[s][0], warp[s, 2:], out_hw, True) - exact[s]).abs().max())
                for s in range(n_held))
    errs = [float((got[s].permute(2, 0, 1).double() - exact[s]).abs().max()) for s in range(n_held)]
    print(f"roi_warp {oh}x{ow}: yardstick fp32 noise {noise:.3e}, bound {4 * noise:.3e}, largest error / allowance "
          f"{max(errs) / (4 * noise):.3f}; kernel max|d| per crop " + " ".join(f"{e:.3e}" for e in errs))
    assert 0.0 < noise < 1e-4
    assert max(errs) <= 4 * noise
    assert all(float(e.abs().max()) > 0.2 for e in exact)             # not vacuous: the crops hold the image
    assert bool((got[n_held - 1] == torch.tensor(GF.CONST)).all())    # the constant frame: the constant exactly
    # the plain restatement of the resampling says the same of these rows
    fr32 = GF._frames()[:, :, 4:4 + H, 5:5 + W].contiguous()
    far = max(float((got[s].permute(2, 0, 1) - AH.roi_warp_ref(fr32, rows[s][0], warp[s, 2:], out_hw)).abs().max())
              for s in range(n_held))
    print(f"roi_warp {oh}x{ow}: largest distance from roi_warp_ref {far:.3e}")
    assert far <= 4 * noise
    # a roll of 0 about a window is that window's resize (two routes to one crop)
    assert float(exact[0].abs().max()) > 0.2


def test_roi_warp_clears_what_is_empty_and_mixes_with_windows(warped):
    out_hw, rows, n_held, warp, outer, amax, plain = warped
    oh, ow = out_hw
    S = outer.shape[0] - 1
    inner = torch.zeros_like(outer, dtype=torch.bool)
    inner[:S, 1:1 + oh, 2:2 + ow, :] = True
    assert bool((outer[~inner] == 7.0).all())          # the border, the extra slot: the sentinel
    y = outer[:S, 1:1 + oh, 2:2 + ow, :]
    assert not bool(torch.isnan(y).any())              # nothing of the NaN surround, no NaN from wild rows
    assert float(y[..., 3].abs().max()) == 0.0
    assert float(y[n_held:n_held + 5].abs().max()) == 0.0             # wholly outside, 1e30, NaN, inf
    assert float(y[n_held + 7:].abs().max()) == 0.0                   # empty slots and the one past n_crops
    for s in (n_held + 5, n_held + 6):                 # the unflagged rows: roi_resize's bits
        assert torch.equal(_bits(y[s]), _bits(plain[s])) and float(y[s].abs().max()) > 0.2
    want = y.abs().amax(dim=(1, 2, 3))
    want[6] = 0.25
    assert n_held == 6 and torch.equal(_bits(amax), _bits(want))
    assert float(amax[:n_held].min()) > 0.0 and float(amax[n_held + 1:n_held + 5].abs().max()) == 0.0


def test_roi_warp_u8_has_the_bits_of_the_float_route():
    out_hw = (9, 130)
    oh, ow = out_hw
    rows, n_held = _warps(out_hw)
    S = len(rows)
    meta = GF._meta([(f, w) for f, _, w in rows], S).to(DEV)
    warp = _warp_rows(S, [(s, c) for s, (_, c, _) in enumerate(rows) if c is not None]).to(DEV)
    n = _i32(S)
    big = _u8_nan_free().to(DEV)
    u8 = big[:, :, 4:4 + H, 5:5 + W].permute(0, 2, 3, 1)               # NCHW slice seen as NHWC
    assert not u8.is_contiguous()

    def run(fn, frames, **kw):
        y, amax = torch.full((S, oh, ow, 4), 7.0, device=DEV), torch.zeros(S, device=DEV)
        fn(frames, meta, n, warp, y, y_amax=amax, **kw)
        return y.cpu(), amax.cpu()
    ref, ref_amax = run(ops.roi_warp, big[:, :, 4:4 + H, 5:5 + W].float())
    got, amax = run(ops.roi_warp_u8, u8)
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(_bits(amax), _bits(ref_amax))
    assert float(ref[:n_held].abs().amax(dim=(1, 2, 3)).min()) > 100.0
    got, amax = run(ops.roi_warp_u8, u8.flip(3), swap_rb=True)          # BGR on channel-flipped frames
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(_bits(amax), _bits(ref_amax))
    # raw * a + b on every pixel of a filled slot (taps outside the frame are raw 0), empty slots
    # exact zeros, y_amax the maximum of what was written
    ing = FrameIngest(norm="imagenet")
    got, amax = run(ops.roi_warp_u8, u8.flip(3), a=ing.a, b=ing.b, swap_rb=True)
    filled = torch.tensor([0 <= f < 3 for f, _, _ in rows])
    want = torch.zeros_like(ref)
    want[filled, :, :, :3] = ref[filled, :, :, :3] * torch.tensor(ing.a) + torch.tensor(ing.b)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(amax), _bits(want.abs().amax(dim=(1, 2, 3))))
    assert float(amax[n_held]) == max(abs(v) for v in ing.b)           # wholly outside the frame: b everywhere


def test_align_wrappers_refuse_bad_buffers():
    meta, n, _ = GF._alloc(4)
    frames = torch.zeros(1, 3, 8, 8, device=DEV)
    y = torch.zeros(4, 12, 12, 4, device=DEV)
    with pytest.raises(ValueError, match="warp"):
        ops.roi_warp(frames, meta, n, torch.zeros(3, 8, device=DEV), y)                           # a row short
    with pytest.raises(ValueError, match="warp"):
        ops.roi_warp(frames, meta, n, torch.zeros(4, 8), y)                                       # on the host
    with pytest.raises(ValueError, match="warp"):
        ops.roi_warp_u8(torch.zeros(1, 8, 8, 3, device=DEV, dtype=torch.uint8), meta, n, torch.zeros(4, 6, device=DEV), y)
    with pytest.raises(ValueError, match="y must be"):
        ops.roi_warp(frames, meta, n, torch.zeros(4, 8, device=DEV), torch.zeros(3, 12, 12, 4, device=DEV))
    kp, pf = torch.zeros(3, 17, 3, device=DEV), torch.zeros(3, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match="warp"):
        ops.face_align_fit(meta, n, n, kp, pf, (112, 112), warp=torch.zeros(3, 8, device=DEV))
    with pytest.raises(ValueError, match="person_face"):
        ops.face_align_fit(meta, n, n, kp, pf[:2], (112, 112), warp=torch.zeros(4, 8, device=DEV))
    with pytest.raises(ValueError, match="scale"):
        ops.face_align_fit(meta, n, n, kp, pf, (112, 112), warp=torch.zeros(4, 8, device=DEV), scale=(2.0, 1.0))
    with pytest.raises(ValueError, match="at least 3"):
        ops.face_align_fit(meta, n, n, kp[:, :2].contiguous(), pf, (112, 112), warp=torch.zeros(4, 8, device=DEV))
    with pytest.raises(ValueError, match="output size"):
        ops.face_align_fit(meta, n, n, kp, pf, (0, 112), warp=torch.zeros(4, 8, device=DEV))


# ---------------------------------------------------------------------------------- PersonRecognition(align=True)
@pytest.fixture(scope="module")
def model(state_dict):
    return CombinedModel(state_dict, device=DEV)


POSE_KW = dict(max_per_frame=2, max_crops=4, box_scale=1.0)
FACE_KW = dict(GF.KW, threshold=0.0)


def _head(kp, s, coef, eye_score=0.9):
    """Person slot s: nose and eyes where ``coef`` puts the template, the ears at the crop's centre."""
    pts = _on_template(coef, (112, 112))
    cx, cy = coef[0] * 56 + coef[1] * 56 + coef[2], coef[3] * 56 + coef[4] * 56 + coef[5]
    kp[s, 0] = torch.tensor([*pts[0], 0.9])
    kp[s, 1] = torch.tensor([*pts[1], eye_score])
    kp[s, 2] = torch.tensor([*pts[2], eye_score])
    kp[s, 3:5] = torch.tensor([cx, cy, 0.9])


@pytest.fixture(scope="module")
def posed(model):
    """The pose stage's output on GF's frames and person boxes, with crafted head keypoints (with
    seeded weights the model's own are arbitrary): person 0 looks out of face A's window rolled by
    20 degrees, person 1 stands at face B with both eyes below kp_thr (its crop falls back to the
    window), person 2 is upright in face C's window."""
    x = GF._model_frames()
    pd, pc = GF._person_dets()
    out_p = dict(TopDownPose(model, **POSE_KW).from_detections(x, pd, pc))
    assert int(out_p["n_crops"]) == 3
    kp = out_p["keypoints"].cpu().clone()
    _head(kp, 0, AH.roll_coef(20, 37.0, (25.0, 26.0), (112, 112)))
    _head(kp, 1, AH.roll_coef(0, 50.0, (85.0, 50.0), (112, 112)), eye_score=0.1)
    _head(kp, 2, AH.roll_coef(0, 41.0, (50.25, 30.125), (112, 112)))
    out_p["keypoints"] = kp.to(DEV)
    return x, out_p


def _gallery():
    g = FaceGallery(dim=512, capacity=8, device=DEV)
    g.add(torch.randn(2, 512, generator=torch.Generator().manual_seed(44)).to(DEV), [5, 6])
    return g


def _tensors(out):
    flat = {f"{k}.{q}": v for k in ("pose", "faces") for q, v in out[k].items()}
    flat.update({k: v for k, v in out.items() if k not in ("pose", "faces")})
    return flat


def test_aligned_person_recognition_equals_the_unfused_route(model, posed, monkeypatch):
    x, out_p = posed
    fd, fc = GF._face_dets()
    gallery = _gallery()
    pr = PersonRecognition(model, gallery, pose=POSE_KW, faces=FACE_KW, align=True)
    pr.from_pose(x, out_p, fd, fc)
    reads = GF._count_reads(monkeypatch)
    out = pr.from_pose(x, out_p, fd, fc)
    assert reads == []                                 # no host read on the default path
    monkeypatch.undo()
    plain = PersonRecognition(model, gallery, pose=POSE_KW, faces=FACE_KW).from_pose(x, out_p, fd, fc)
    assert set(out) == set(plain) | {"face_warp"} and set(out["faces"]) == set(plain["faces"])
    assert torch.equal(out["person_face"], plain["person_face"]) and torch.equal(out["match_status"], plain["match_status"])
    assert out["person_face"].tolist() == [0, 1, 2, -1]
    # the unfused route: list, match with nobody identified, fit, warp, trunk, AdaFace, gallery, join
    e = model.engine
    cap, P = 5, 4
    meta, n, st = GF._alloc(cap)
    ops.roi_select(fd, fc, x.shape[2:], (112, 112), crop_meta=meta, n_crops=n, status=st, score_thr=pr.faces.score_thr,
                   max_per_frame=3, min_size=pr.faces.min_size, box_scale=(1.0, 1.0), pad=pr.faces.pad)
    assert _same(out["faces"]["crop_meta"], meta) and int(n) == 3
    bufs = dict(face_slot=torch.empty(P, device=DEV, dtype=torch.int32),
                person_ident=torch.empty(P, device=DEV, dtype=torch.int64),
                person_score=torch.empty(P, device=DEV), status=torch.empty(2, device=DEV, dtype=torch.int32))
    ops.face_person_match(out_p["crop_meta"], out_p["n_crops"], out_p["keypoints"], meta, n,
                          torch.full((cap,), -1, device=DEV, dtype=torch.int64), torch.full((cap,), -INF, device=DEV), 2,
                          kp_thr=0.3, head_kpts=5, **bufs)
    assert torch.equal(out["person_face"], bufs["face_slot"])
    warp = ops.face_align_fit(meta, n, out_p["n_crops"], out_p["keypoints"], bufs["face_slot"], (112, 112),
                              warp=torch.zeros(cap, 8, device=DEV))
    assert _same(out["face_warp"], warp)
    assert warp.cpu().view(torch.int32)[:, :2].tolist() == [[1, 0], [0, 0], [1, 2], [0, 0], [0, 0]]
    ref = AH.face_align_fit_ref(meta.cpu(), 3, 3, out_p["keypoints"].cpu(), bufs["face_slot"].cpu(), (112, 112))
    assert torch.equal(_bits(warp[:, :2].cpu()), _bits(ref[:, :2]))
    y = torch.zeros(cap, 112, 112, 4, device=DEV)
    ops.roi_warp(x, meta, n, warp, y)
    crops = y[:3, :, :, :3].permute(0, 3, 1, 2).contiguous()
    emb, norms = e.adaface(e.trunk(crops))
    assert _same(out["faces"]["embeddings"][:3], emb) and _same(out["faces"]["norms"][:3], norms.view(3))
    assert float(out["faces"]["embeddings"][3:].abs().max()) == 0.0
    ident, score = gallery.identify(emb, 0.0)
    assert torch.equal(out["faces"]["ident"][:3], ident) and _same(out["faces"]["score"][:3], score)
    assert torch.equal(out["person_ident"][:3], ident) and _same(out["person_score"][:3], score)
    assert int(out["person_ident"][3]) == -1 and float(out["person_score"][3]) == -INF
    # the face that fell back has the unaligned route's bits; the aligned ones were resampled anew
    pe, oe = plain["faces"]["embeddings"], out["faces"]["embeddings"]
    assert _same(pe[1], oe[1]) and not torch.equal(pe[0], oe[0]) and not torch.equal(pe[2], oe[2])
    people = PersonRecognition.results(out)
    assert [[p["face_aligned"] for p in fr] for fr in people] == [[True, False], [True]]
    assert [[p["ident"] for p in fr] for fr in people] == [ident[:2].tolist(), ident[2:].tolist()]
    # compact: one read, the same bits in [:n]
    pr_c = PersonRecognition(model, gallery, pose=POSE_KW, faces=dict(FACE_KW, compact=True), align=True)
    got = pr_c.from_pose(x, out_p, fd, fc)
    a, b = _tensors(out), _tensors(got)
    assert set(a) == set(b) and all(_same(a[k], b[k]) for k in a), [k for k in a if not _same(a[k], b[k])]


def test_alignment_without_usable_keypoints_is_the_plain_route_bit_for_bit(model, posed):
    x, out_p = posed
    fd, fc = GF._face_dets()
    low = dict(out_p)
    low["keypoints"] = out_p["keypoints"].clone()
    low["keypoints"][:, :, 2] = 0.25                   # every score below kp_thr = 0.3
    gallery = _gallery()
    plain = PersonRecognition(model, gallery, pose=POSE_KW, faces=FACE_KW).from_pose(x, low, fd, fc)
    out = PersonRecognition(model, gallery, pose=POSE_KW, faces=FACE_KW, align=True).from_pose(x, low, fd, fc)
    assert float(out["face_warp"].abs().max()) == 0.0
    a, b = _tensors(plain), _tensors(out)
    assert set(b) == set(a) | {"face_warp"}
    assert all(_same(a[k], b[k]) for k in a), [k for k in a if not _same(a[k], b[k])]
    assert int(plain["faces"]["n_crops"]) == 3 and bool((plain["person_face"][:3] >= 0).all())


def test_enrolled_aligned_faces_are_identified(model, posed):
    x, out_p = posed
    fd, fc = GF._face_dets()
    gallery = FaceGallery(dim=512, capacity=8, device=DEV)
    pr = PersonRecognition(model, gallery, pose=POSE_KW, faces=FACE_KW, align=True)
    # the best face of each frame (A, C), aligned as the probes will be; a third frame without a face
    x3 = torch.cat([x, x[:1]])
    p3 = {k: v for k, v in out_p.items()}
    ed, ec = GF._dets([[(*GF.BOX_A, 0.9), (*GF.BOX_B, 0.7)], [(*GF.BOX_C, 0.6)], [(*GF.BOX_D, 0.2)]])
    assert pr.enrol_pose(x3, p3, ed, ec, [21, 22, 23]) == [2] and len(gallery) == 2
    out = pr.from_pose(x, out_p, fd, fc)
    emb = out["faces"]["embeddings"][:3].cpu()
    s64 = F.normalize(emb.double(), dim=1) @ F.normalize(emb[[0, 2]].double(), dim=1).t()
    s32 = F.normalize(emb, dim=1) @ F.normalize(emb[[0, 2]], dim=1).t()
    bound = 4 * float((s32.double() - s64).abs().max())
    score = out["person_score"].cpu()
    print(f"aligned enrol: bound {bound:.3e}, enrolled scores {float(score[0]):.7f} {float(score[2]):.7f}, "
          f"the unenrolled face's best {float(s64[1].max()):.6f}")
    assert out["person_ident"].tolist()[:3:2] == [21, 22]
    assert abs(float(score[0]) - 1) <= bound and abs(float(score[2]) - 1) <= bound
    assert float(s64[1].max()) < 1 - 4 * bound         # the third face is somebody else
    assert out["face_warp"].cpu().view(torch.int32)[:3, 0].tolist() == [1, 0, 1]
    # without alignment the same enrolment is a different crop: the geometry is what was enrolled
    plain = PersonRecognition(model, gallery, pose=POSE_KW, faces=FACE_KW).from_pose(x, out_p, fd, fc)
    assert float(plain["person_score"][0]) < 1 - 4 * bound
