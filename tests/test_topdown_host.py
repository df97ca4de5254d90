"""CPU: the top-down pose stage (prpe.topdown, csrc/topdown.hip) as far as the host goes -- the
ABI table, a pure-torch restatement of the crop list rule and of the window arithmetic
(``window_ref`` / ``select_ref``, which tests/test_gpu_topdown.py holds the kernel to, bit for
bit), ``TopDownPose.results`` and the argument checks of the ops wrappers."""
import os
import re

import pytest
import torch

from conftest import ROOT

from prpe import _lib

A = torch.tensor(192.0 / 256.0, dtype=torch.float32)          # the crop's aspect, 0.75 exactly


def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def window_ref(x1, y1, x2, y2, pad):
    """(x0, y0, w, h) of include/prpe.h's window, every step one fp32 operation (0-dim float32
    tensors: torch's CPU arithmetic rounds each of them once and fuses nothing)."""
    x1, y1, x2, y2, pad = (_f(v) for v in (x1, y1, x2, y2, pad))
    cx, cy = (x1 + x2) * 0.5, (y1 + y2) * 0.5
    w, h = x2 - x1, y2 - y1
    if bool(w > A * h):
        h = w / A
    else:
        w = h * A
    w, h = w * pad, h * pad
    return cx - 0.5 * w, cy - 0.5 * h, w, h


def select_ref(dets, counts, score_thr=0.25, max_per_frame=8, min_size=4.0, box_scale=(1.0, 1.0), pad=1.25,
               max_crops=8):
    """prpe_crop_select on the host: (crop_meta [max_crops, 8] float32, n_crops, status)."""
    dets = dets.float().cpu()
    sx, sy = _f(box_scale[0]), _f(box_scale[1])
    thr, mins = _f(score_thr), _f(min_size)
    rows, status = [], 0
    for b, c in enumerate(int(v) for v in counts):
        if c < 0:
            status |= 1                               # NMS candidate overflow: nothing from b
            continue
        pre = 0                                       # the first rows with score >= thr, at most max_per_frame
        while pre < min(c, dets.shape[1], max_per_frame) and bool(dets[b, pre, 4] >= thr):
            pre += 1
        for r in range(pre):
            x1, y1, x2, y2 = dets[b, r, 0] * sx, dets[b, r, 1] * sy, dets[b, r, 2] * sx, dets[b, r, 3] * sy
            if not all(bool(torch.isfinite(v)) for v in (x1, y1, x2, y2)):
                continue
            if not bool(x2 - x1 >= mins) or not bool(y2 - y1 >= mins):
                continue
            win = window_ref(x1, y1, x2, y2, pad)
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


def _dets(frames):
    """[[ (x1, y1, x2, y2, score), ... ], ...] -> (dets [B, max_det, 6] with NaN in unused rows,
    as torch.empty may leave them, counts [B])."""
    max_det = max(1, max(len(f) for f in frames))
    d = torch.full((len(frames), max_det, 6), float("nan"))
    for b, f in enumerate(frames):
        for r, row in enumerate(f):
            d[b, r, :5] = torch.tensor(row, dtype=torch.float32)
            d[b, r, 5] = 0.0
    return d, torch.tensor([len(f) for f in frames], dtype=torch.int32)


def _frames_rows(meta, n):
    ints = meta.view(torch.int32)
    return [(int(ints[s, 0]), int(ints[s, 1])) for s in range(n)]


# ---------------------------------------------------------------------------------- ABI
def test_abi_table_has_the_topdown_entry_points():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert _lib.ABI_VERSION == 12
    assert int(re.search(r"#define PRPE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for name, nargs in (("prpe_crop_select", 17), ("prpe_crop_resize", 6), ("prpe_crop_keypoints", 9)):
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/prpe.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().prpe_abi_version() == 12


def test_library_rejects_bad_topdown_arguments_before_launch():
    L = _lib.lib()
    p = 0x1000
    assert L.prpe_crop_select(None, p, 1, 1, 0.25, 8, 4.0, 1.0, 1.0, 64, 64, 1.25, 4, p, p, p, None) == -22
    assert L.prpe_crop_select(p, p, 1, 1, 0.25, 8, 4.0, 1.0, 1.0, 64, 64, 1.25, 0, p, p, p, None) == -22   # no slot
    assert L.prpe_crop_select(p, p, 1, 1, 0.25, 8, 4.0, 1.0, 1.0, 64, 64, 0.0, 4, p, p, p, None) == -22    # pad 0
    assert L.prpe_crop_select(p, p, 1, 1, 0.25, 8, 4.0, float("nan"), 1.0, 64, 64, 1.25, 4, p, p, p, None) == -22
    v4 = _lib.View(p, 1, 8, 8, 4, 256, 32, 4, 1)
    import ctypes as C
    assert L.prpe_crop_resize(C.byref(v4), p, p, 1, p, None) == -22                  # 4 channels
    v3 = _lib.View(p, 1, 8, 8, 3, 192, 24, 3, 1)
    assert L.prpe_crop_resize(C.byref(v3), p, p, 1, p + 4, None) == -22              # unaligned buffer
    assert L.prpe_crop_resize(C.byref(v3), p, None, 1, p, None) == -22
    assert L.prpe_crop_keypoints(p, p, 5, 17, p, p, 4, p, None) == -22               # more rows than slots
    assert L.prpe_crop_keypoints(p, p, 0, 17, p, p, 4, p, None) == -22


# ---------------------------------------------------------------------------------- the rule
def test_window_arithmetic_on_hand_cases():
    # tall box 40 x 100: w grows to 0.75 * 100 = 75, both * 1.25, centred on (30, 70)
    assert [float(v) for v in window_ref(10, 20, 50, 120, 1.25)] == [-16.875, 7.5, 93.75, 125.0]
    # wide box 120 x 40: h grows to 120 / 0.75 = 160
    assert [float(v) for v in window_ref(0, 0, 120, 40, 1.25)] == [-15.0, -80.0, 150.0, 200.0]
    # exactly 3:4 and pad 1: the window is the box
    assert [float(v) for v in window_ref(8, 16, 200, 272, 1.0)] == [8.0, 16.0, 192.0, 256.0]
    # every step rounds to fp32: the same chain in float64 gives other bits
    x0, y0, w, h = window_ref(0, 0, 100, 10, 1.25)
    assert h.dtype == torch.float32 and float(h) != 100 / 0.75 * 1.25
    assert abs(float(h) - 100 / 0.75 * 1.25) < 1e-4 and float(w) == 125.0 and float(x0) == -12.5


def test_select_score_threshold_and_max_per_frame():
    d, c = _dets([[(0, 0, 30, 40, 0.9), (5, 5, 35, 45, 0.6), (9, 9, 39, 49, 0.2), (1, 1, 31, 41, 0.1)],
                  [(0, 0, 30, 40, 0.5), (5, 5, 35, 45, 0.4), (9, 9, 39, 49, 0.3)]])
    meta, n, st = select_ref(d, c, score_thr=0.25, max_per_frame=8, max_crops=8)
    assert _frames_rows(meta, n) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)] and st == 0
    meta, n, st = select_ref(d, c, score_thr=0.25, max_per_frame=2, max_crops=8)
    assert _frames_rows(meta, n) == [(0, 0), (0, 1), (1, 0), (1, 1)] and st == 0
    assert [float(v) for v in meta[:n, 6]] == [float(_f(v)) for v in (0.9, 0.6, 0.5, 0.4)]
    assert int(meta.view(torch.int32)[n, 0]) == -1 and float(meta[n:, 1:].abs().sum()) == 0.0
    meta, n, st = select_ref(d, c, score_thr=0.95)
    assert n == 0 and st == 0 and bool((meta.view(torch.int32)[:, 0] == -1).all())


def test_select_skips_degenerate_and_nan_boxes():
    nan, inf = float("nan"), float("inf")
    d, c = _dets([[(0, 0, 30, 40, 0.9), (10, 10, 12, 80, 0.8), (nan, 0, 30, 40, 0.7), (0, 0, inf, 40, 0.65),
                   (20, 20, 60, 23.9, 0.6), (2, 2, 6, 6, 0.5)]])
    meta, n, st = select_ref(d, c, min_size=4.0)
    assert _frames_rows(meta, n) == [(0, 0), (0, 5)] and st == 0          # 2 wide, NaN, inf, 3.9 high: skipped
    # a skipped row still uses up one of the max_per_frame candidates
    meta, n, st = select_ref(d, c, min_size=4.0, max_per_frame=5)
    assert _frames_rows(meta, n) == [(0, 0)]
    # min_size is in frame pixels, after the scale
    meta, n, st = select_ref(d, c, min_size=4.0, box_scale=(2.0, 2.0))
    assert _frames_rows(meta, n) == [(0, 0), (0, 1), (0, 4), (0, 5)]
    assert [float(v) for v in meta[0, 2:6]] == [float(v) for v in window_ref(0, 0, 60, 80, 1.25)]


def test_select_negative_count_and_truncation_set_status():
    d, c = _dets([[(0, 0, 30, 40, 0.9), (1, 1, 31, 41, 0.8)], [(0, 0, 30, 40, 0.9)],
                  [(0, 0, 30, 40, 0.7), (2, 2, 32, 42, 0.6), (3, 3, 33, 43, 0.5)]])
    c[1] = -1
    meta, n, st = select_ref(d, c, max_crops=8)
    assert _frames_rows(meta, n) == [(0, 0), (0, 1), (2, 0), (2, 1), (2, 2)] and st == 1
    meta, n, st = select_ref(d, c, max_crops=3)
    assert _frames_rows(meta, n) == [(0, 0), (0, 1), (2, 0)] and st == 3  # dropped from the end
    c[1] = 1
    meta, n, st = select_ref(d, c, max_crops=6)
    assert n == 6 and st == 0                                            # exactly full is no overflow
    assert _frames_rows(meta, n) == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (2, 2)]


# ---------------------------------------------------------------------------------- the edges
NAN, INF = float("nan"), float("inf")


def _below(v):
    """The next fp32 below ``v`` (a Python float)."""
    return float(torch.nextafter(_f(v), _f(-INF)))


def _above(v):
    return float(torch.nextafter(_f(v), _f(INF)))


def select_edge_cases():
    """The crop_select edge cases that tests/test_gpu_framestages.py sends to the kernel: name ->
    (dets, counts, keyword arguments, expected n_crops, expected status, expected (frame, row)
    list). The expectations are literals worked out by hand from include/prpe.h's rule; this file
    holds ``select_ref`` and an independent numpy statement of the rule to them."""
    cases = {}
    ok = (0.0, 0.0, 30.0, 40.0)
    # -- the prefix: >= thr keeps, the next fp32 below ends it (the 0.9 behind it is never
    # reached), a NaN score ends it; counts above max_det are clamped to the rows there are
    thr = 0.25
    frames = [[(*ok, _above(thr)), (*ok, thr), (*ok, _below(thr)), (*ok, 0.9)],
              [(*ok, 0.9), (*ok, NAN), (*ok, 0.9)],
              [(*ok, 0.9), (1.0, 1.0, 31.0, 41.0, 0.8), (2.0, 2.0, 32.0, 42.0, 0.7), (3.0, 3.0, 33.0, 43.0, 0.6)],
              [(5.0, 5.0, 35.0, 45.0, 0.5)] * 4]
    d, c = _dets(frames)
    c[2] = 100                                        # > max_det = 4: frame 3's rows are not frame 2's
    cases["prefix"] = (d, c, dict(score_thr=thr, max_per_frame=8, max_crops=16), 11, 0,
                       [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0), (3, 1), (3, 2), (3, 3)])
    # -- min_size: a side exactly min_size is kept, the next fp32 below is dropped (either side)
    ms = 4.0
    frames = [[(10.0, 10.0, 14.0, 50.0, 0.9), (0.0, 10.0, _below(ms), 50.0, 0.8), (10.0, 10.0, 50.0, 14.0, 0.7),
               (10.0, 0.0, 50.0, _below(ms), 0.6), (10.0, 10.0, 14.0, 14.0, 0.5)]]
    d, c = _dets(frames)
    cases["min_size"] = (d, c, dict(min_size=ms, max_crops=8), 3, 0, [(0, 0), (0, 2), (0, 4)])
    # -- the aspect branch under box_scale_x != box_scale_y: in frame pixels the boxes are
    # 30 x 40 (w == a h: the else branch, which leaves both sides), 30.75 x 40 (w > a h: h grows)
    # and 28.5 x 40 (w < a h: w grows); with the scales exchanged all three would be wide
    frames = [[(10.0, 20.0, 30.0, 100.0, 0.9), (10.0, 20.0, 30.5, 100.0, 0.8), (10.0, 20.0, 29.0, 100.0, 0.7)]]
    d, c = _dets(frames)
    cases["aspect"] = (d, c, dict(box_scale=(1.5, 0.5), pad=1.0, max_crops=3), 3, 0, [(0, 0), (0, 1), (0, 2)])
    # -- +-inf coordinates, and a box that is finite after the scale (w = 2.2e38) whose window
    # overflows under pad (h = w / a = 2.93e38 is finite, h * 1.25 is inf): both are skipped and
    # both use up a place among max_per_frame = 3, so row 3 of each frame is never a candidate
    big = 1.1e38
    frames = [[(-INF, 0.0, 30.0, 40.0, 0.9), (0.0, 0.0, 30.0, INF, 0.8), ok + (0.7,), ok + (0.6,)],
              [(-big, 0.0, big, 40.0, 0.9), ok + (0.8,), (0.0, -INF, 30.0, INF, 0.7), ok + (0.6,)]]
    d, c = _dets(frames)
    cases["nonfinite"] = (d, c, dict(max_per_frame=3, max_crops=4), 2, 0, [(0, 2), (1, 1)])
    # -- every slot padded / none padded
    d, c = _dets([[ok + (0.2,)], [ok + (0.1,)], []])
    cases["none"] = (d, c, dict(max_crops=5), 0, 0, [])
    d, c = _dets([[ok + (0.9,), ok + (0.8,)], [], [ok + (0.7,)]])
    cases["exactly_full"] = (d, c, dict(max_crops=3), 3, 0, [(0, 0), (0, 1), (2, 0)])
    # -- more frames than threads: counts b % 3 give 255 crops from frames 0..255, so a list of
    # 400 slots overflows in the second chunk of 256 frames (its last slot is frame 400's only
    # row: 133 whole cycles of three frames end at frame 398 with 399 crops)
    B = 600
    xy = (torch.arange(B * 3 * 2, dtype=torch.float32).view(B, 3, 2) % 37) * 0.5
    d = torch.cat([xy, xy + 20.0, torch.full((B, 3, 1), 0.5), torch.zeros(B, 3, 1)], 2)
    c = (torch.arange(B) % 3).int()
    rows = [(b, r) for b in range(B) for r in range(b % 3)]
    cases["late_overflow"] = (d, c, dict(max_per_frame=3, max_crops=400), 400, 2, rows[:400])
    assert rows[399] == (400, 0) and len(rows) == 600
    # -- counts < 0 at b >= 256 (the second pass of the chunk loop): status bit 0 alone, and
    # nothing from that frame
    B = 300
    d = d[:B, :1].clone()
    c = torch.ones(B, dtype=torch.int32)
    c[280] = -1
    cases["late_negative_count"] = (d, c, dict(max_crops=300), 299, 1, [(b, 0) for b in range(B) if b != 280])
    return cases


def select_plain(dets, counts, score_thr=0.25, max_per_frame=8, min_size=4.0, box_scale=(1.0, 1.0), pad=1.25,
                 max_crops=8):
    """include/prpe.h's rule once more, on numpy float32 scalars (each operation rounds once) and
    with math.isfinite: written apart from ``select_ref`` / ``window_ref`` and sharing no code
    with them. Returns ([(frame, row, x0, y0, w, h, score)], status)."""
    import math
    import numpy as np
    f = np.float32
    d = dets.numpy().astype(np.float32)
    out, status = [], 0
    with np.errstate(all="ignore"):
        for b in range(d.shape[0]):
            c = int(counts[b])
            if c < 0:
                status |= 1
                continue
            tried = 0
            for r in range(min(c, d.shape[1])):
                if tried == max_per_frame or not d[b, r, 4] >= f(score_thr):
                    break
                tried += 1
                x1, x2 = d[b, r, 0] * f(box_scale[0]), d[b, r, 2] * f(box_scale[0])
                y1, y2 = d[b, r, 1] * f(box_scale[1]), d[b, r, 3] * f(box_scale[1])
                if not all(math.isfinite(v) for v in (x1, y1, x2, y2)):
                    continue
                w, h = f(x2 - x1), f(y2 - y1)
                if not (w >= f(min_size) and h >= f(min_size)):
                    continue
                if w * f(4.0) > h * f(3.0):           # w / h > 3 / 4 (exact for the sizes used here)
                    h = f(w / f(0.75))
                else:
                    w = f(h * f(0.75))
                w, h = f(w * f(pad)), f(h * f(pad))
                x0 = f(f(f(x1 + x2) * f(0.5)) - f(f(0.5) * w))
                y0 = f(f(f(y1 + y2) * f(0.5)) - f(f(0.5) * h))
                if all(math.isfinite(v) for v in (x0, y0, w, h)):
                    out.append((b, r, x0, y0, w, h, d[b, r, 4]))
    if len(out) > max_crops:
        status |= 2
    return out[:max_crops], status


@pytest.mark.parametrize("name", sorted(select_edge_cases()))
def test_select_ref_at_the_edges_equals_the_plain_statement(name):
    """``select_ref`` at the edges the GPU test sends to the kernel, against ``select_plain`` bit
    for bit and against the literal expectations of ``select_edge_cases``. The rule is this
    project's own (include/prpe.h): the reference has no crop list, so the header decides --
    ``>=`` at both thresholds (a NaN compares false and ends the prefix / drops the box), ``>`` in
    the aspect test, a box or window with a non-finite field skipped after it took its place."""
    import numpy as np
    dets, counts, kw, want_n, want_status, want_rows = select_edge_cases()[name]
    meta, n, status = select_ref(dets, counts, **kw)
    rows, status_plain = select_plain(dets, counts, **kw)
    assert (n, status) == (want_n, want_status) == (len(rows), status_plain)
    assert _frames_rows(meta, n) == want_rows == [(b, r) for b, r, *_ in rows]
    for s, row in enumerate(rows):
        assert np.array_equal(meta[s, 2:7].numpy().view(np.int32), np.array(row[2:], np.float32).view(np.int32)), s
    ints = meta.view(torch.int32)
    assert bool((ints[n:, 0] == -1).all()) and not bool(ints[n:, 1:].any()) and not bool(ints[:n, 7].any())
    assert bool(torch.isfinite(meta[:n, 2:7]).all())


def test_window_ref_at_the_aspect_equality_and_under_unequal_scales():
    """The windows of the ``aspect`` case by hand: 30 x 40 stays (w == a h takes the else branch,
    w = h a = 30), 30.75 x 40 grows to 30.75 x 41, 28.5 x 40 grows to 30 x 40 about its own
    centre."""
    dets, counts, kw, *_ = select_edge_cases()["aspect"]
    meta, n, _ = select_ref(dets, counts, **kw)
    assert [float(v) for v in meta[0, 2:6]] == [15.0, 10.0, 30.0, 40.0]
    assert [float(v) for v in meta[1, 2:6]] == [15.0, 9.5, 30.75, 41.0]
    assert [float(v) for v in meta[2, 2:6]] == [14.25, 10.0, 30.0, 40.0]


# ---------------------------------------------------------------------------------- host helpers
def test_results_formatting():
    from prpe import TopDownPose
    d, c = _dets([[(10, 20, 50, 120, 0.9)], [], [(0, 0, 120, 40, 0.8), (8, 16, 200, 272, 0.7)]])
    meta, n, st = select_ref(d, c, max_crops=5)
    kp = torch.zeros(5, 17, 3)
    kp[:n] = torch.arange(n * 51, dtype=torch.float32).view(n, 17, 3)
    out = {"dets": d, "counts": c, "crop_meta": meta, "n_crops": torch.tensor([n], dtype=torch.int32),
           "status": torch.tensor([st], dtype=torch.int32), "keypoints": kp}
    people = TopDownPose.results(out)
    assert [len(p) for p in people] == [1, 0, 2]
    p = people[0][0]
    assert p["box"] == [-16.875, 7.5, -16.875 + 93.75, 7.5 + 125.0] and p["score"] == float(_f(0.9)) and p["row"] == 0
    assert people[2][1]["row"] == 1 and people[2][1]["score"] == float(_f(0.7))
    assert people[2][1]["keypoints"].shape == (17, 3) and torch.equal(people[2][1]["keypoints"], kp[2])


def test_ops_validate_arguments_before_any_launch():
    """Host tensors, wrong dtypes, strided or short buffers raise ValueError in the wrappers (no
    device is needed to get there, and nothing is launched)."""
    from prpe import ops
    for name in ("crop_select", "crop_resize", "crop_keypoints"):
        assert callable(getattr(ops, name))
    d, c = _dets([[(0, 0, 30, 40, 0.9)]])
    meta = torch.zeros(4, 8)
    n = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="dets"):
        ops.crop_select(d, c, (64, 64), crop_meta=meta, n_crops=n, status=n.clone())       # host tensors
    with pytest.raises(ValueError, match="dets"):
        ops.crop_select(d[..., :5], c, (64, 64), crop_meta=meta, n_crops=n, status=n.clone())
    with pytest.raises(ValueError, match="frames"):
        ops.crop_resize(torch.zeros(1, 3, 8, 8), meta, n, torch.zeros(4, 260, 196, 4))
    with pytest.raises(ValueError, match="coords"):
        ops.crop_keypoints(torch.zeros(4, 17, 3), torch.zeros(4, 17), meta, n, torch.zeros(4, 17, 3))
    # _check_dev: what every buffer goes through (dtype, device, contiguity, exact shape / capacity)
    with pytest.raises(ValueError, match="crop_meta"):
        ops._check_dev("t", "crop_meta", torch.zeros(3, 8), torch.float32, (4, 8))         # host, short
    with pytest.raises(ValueError, match="counts"):
        ops._check_dev("t", "counts", torch.zeros(2, dtype=torch.int64), torch.int32, (2,))
    with pytest.raises(ValueError, match="crops"):
        ops._check_dev("t", "crops", torch.zeros(4, 260, 196, 8)[..., :4], torch.float32, (4, 260, 196, 4))


def test_crop_buffer_is_a_kind_of_its_own():
    """Engine.crop_pix4 does not share vit_pix4's kind: alternating whole-frame pose (batch B) and
    top-down pose (batch max_crops) keeps both buffers."""
    from prpe import engine as E
    e = E.Engine({}, device="cpu")
    a, b = e.vit_pix4(2), e.crop_pix4(5)
    assert a.shape == (2, 260, 196, 4) and b.shape == (5, 260, 196, 4)
    assert e.vit_pix4(2) is a and e.crop_pix4(5) is b and e.vit_pix4(2) is a
    pix = e.pix4_interior(b[:3])
    assert pix.t.shape == (3, 256, 192, 3) and pix.pix4.data_ptr() == b.data_ptr()
    assert pix.t.data_ptr() == b[0, 2, 2].data_ptr()
