"""GPU: the detection evaluation path -- prpe_nms, prpe_det_metrics_update / _compute and
prpe_det_eval_loss -- branch by branch against the oracle's restatements (oracle/model_ref.py:
non_max_suppression / nms_single, DetectionMetricsRef, compute_iou_ref, detection_eval_loss_ref).
The oracle is the yardstick, never the kernels; every input comes from a seeded torch.Generator
or is written out by hand, no golden file is read.

Bars
* NMS: rows and counts bit-exact, rows past the count all zero, layout 1 (the transposed input)
  gives the same bits as layout 0.
* metrics update: counters equal, (score, best IoU) records bit-equal in order (a NaN is a NaN).
* metrics compute: precision / recall / f1 exact; the APs within 1e-6 * max(1, |v|) up to 2048
  records and 1e-5 * max(1, |v|) above (fp32 summation order of torch.trapz against the kernel's
  per-tile double sums), the tolerances test_gpu_evalsteps.py already uses.
* eval loss: the reference in fp64 on the same fp32 inputs, 2e-5 * max(1, |v|) per term and for
  the batch loss (fp32 libm and reduction order); a NaN term is NaN on both sides; an image the
  reference skips has per_image[b, 0] == 0. So that fp32 and fp64 take the same decisions, each
  case asserts on the reference alone that no best IoU lies within 1e-4 of 0.5 and no maximum
  score within 1e-5 of 0.01 (a condition on the seeded inputs).

The input builders below are plain cached functions: they assert the conditions that depend on
the oracle alone (kept counts, max_nms changing the kept set, the margins), so those can be run
without a device.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import model_ref as R
from prpe import ops
from prpe._lib import PrpeError
from prpe.evalsteps import DetectionMetricsDevice, detection_eval_loss

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    """fp32 tensors equal bit for bit; NaN matches NaN (the sign of a generated NaN differs
    between the host's and the device's arithmetic)."""
    a, b = a.contiguous().float(), b.contiguous().float()
    if a.shape != b.shape:
        return False
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


# ============================================================================= 1. NMS
def _nms_input(seed, B, N, nc, canvas, lo=0.3, hi=1.0, side=(8.0, 60.0)):
    """[B, 4+nc, N]: centres over a canvas x canvas area, sides 8..60, scores in [lo, hi)."""
    g = torch.Generator().manual_seed(seed)
    cxy = torch.rand(B, 2, N, generator=g) * canvas
    wh = torch.rand(B, 2, N, generator=g) * (side[1] - side[0]) + side[0]
    sc = torch.rand(B, nc, N, generator=g) * (hi - lo) + lo
    return torch.cat([cxy, wh, sc], 1).contiguous()


def _nms_check(inp, conf, iou, max_det=300, max_nms=30000, ref=None):
    """Both layouts against the oracle; returns the oracle's list."""
    if ref is None:
        ref = R.non_max_suppression(inp, conf, iou, max_det=max_det, max_nms=max_nms)
    for layout in (0, 1):
        x = inp if layout == 0 else inp.transpose(1, 2).contiguous()
        out, cnt = ops.nms(x.cuda(), layout, conf, iou, max_nms, max_det)
        torch.cuda.synchronize()
        out, cnt = out.cpu(), cnt.cpu().tolist()
        assert out.shape == (inp.shape[0], max_det, 6)
        assert cnt == [len(r) for r in ref], (layout, cnt, [len(r) for r in ref])
        for i, r in enumerate(ref):
            assert _same_bits(out[i, :cnt[i]], r.reshape(-1, 6)), (layout, i)
            assert bool((out[i, cnt[i]:].view(torch.int32) == 0).all()), (layout, i)
    return ref


@functools.lru_cache(maxsize=None)
def _nms_path_case(nc, N):
    """Every score passes conf = 0.25, so all N*nc pairs are candidates. Sides 40..60 on a canvas
    wide enough that the kept list spans several 64-lane slices, and small enough that it never
    reaches max_det = 1024: the greedy pass walks the whole sorted list."""
    inp = _nms_input(1000 * nc + N, 1, N, nc, 400.0 if nc == 1 else 200.0, side=(40.0, 60.0))
    ref = R.non_max_suppression(inp, 0.25, 0.5, max_det=1024)
    assert bool((inp[:, 4:] > 0.25).all())
    assert all(64 < len(r) < 1024 for r in ref), [len(r) for r in ref]
    return inp, ref


# N*nc = 16384 is the last size of the LDS path (a full 16384-key bitonic sort), 16385 / 16388
# the first of the global (radix sort) path
@pytest.mark.parametrize("nc,N", [(1, 16384), (1, 16385), (4, 4096), (4, 4097)])
def test_nms_path_switch(nc, N):
    inp, ref = _nms_path_case(nc, N)
    _nms_check(inp, 0.25, 0.5, max_det=1024, ref=ref)


@functools.lru_cache(maxsize=None)
def _nms_count_case(t):
    """N = 1500 (two enumerate rounds of 1024 with a tail), exactly t scores above conf per
    image, on both sides of anchor 1024."""
    B, N = 2, 1500
    inp = _nms_input(77 + t, B, N, 1, 500.0)
    g = torch.Generator().manual_seed(t)
    passing = inp[:, 4].clone()
    inp[:, 4] = 0.1
    for b in range(B):
        perm = torch.randperm(N, generator=g)
        must = [1024, 1023, 0, N - 1][:min(t, 4)] if b == 0 else [1024, 1023][:min(t, 2)]
        rest = [int(i) for i in perm if int(i) not in must]
        idx = torch.tensor(must + rest[:t - len(must)], dtype=torch.int64)
        inp[b, 4, idx] = passing[b, idx]
        assert int((inp[b, 4] > 0.25).sum()) == t
        if t >= 2:
            assert int((idx < 1024).sum()) > 0 and int((idx >= 1024).sum()) > 0
    return inp


# 0 / 1: the bitonic padding at total = 0 and P = 1; 2, 256, 1024: total a power of two;
# 257, 1025: a power of two + 1; 255 / 256 / 257: around the 256-candidate greedy chunk
@pytest.mark.parametrize("t", [0, 1, 2, 255, 256, 257, 1024, 1025])
def test_nms_candidate_counts_lds_path(t):
    ref = _nms_check(_nms_count_case(t), 0.25, 0.5, max_det=1024)
    if t:
        assert all(0 < len(r) <= t for r in ref)
    if t >= 255:
        assert all(len(r) < t for r in ref)          # something is suppressed


@functools.lru_cache(maxsize=None)
def _nms_max_nms_case():
    inp = _nms_input(31, 1, 2000, 1, 150.0)
    refs = {m: R.non_max_suppression(inp, 0.25, 0.5, max_det=1024, max_nms=m) for m in (1, 256, 257, 1999)}
    kept = {m: [tuple(row) for row in r[0].tolist()] for m, r in refs.items()}
    assert len(kept[1]) == 1
    # truncation happens before the greedy pass: the kept set grows with max_nms
    assert set(kept[1]) < set(kept[256]) and set(kept[257]) < set(kept[1999])
    assert len(kept[1999]) < 1024                    # not cut by max_det
    return inp, refs


@pytest.mark.parametrize("max_nms", [1, 256, 257, 1999])
def test_nms_max_nms_lds_path(max_nms):
    inp, refs = _nms_max_nms_case()
    _nms_check(inp, 0.25, 0.5, max_det=1024, max_nms=max_nms, ref=refs[max_nms])


@functools.lru_cache(maxsize=None)
def _nms_max_det_case():
    """3000 boxes thinly spread: the oracle alone keeps at least 1024."""
    inp = _nms_input(53, 1, 3000, 1, 4000.0)
    assert len(R.non_max_suppression(inp, 0.25, 0.5, max_det=3000)[0]) >= 1024
    return inp


@pytest.mark.parametrize("max_det", [1, 64, 65, 1024])
def test_nms_max_det(max_det):
    inp = _nms_max_det_case()
    ref = _nms_check(inp, 0.25, 0.5, max_det=max_det)
    assert len(ref[0]) == max_det


def test_nms_max_det_above_the_kept_list_is_refused():
    with pytest.raises(PrpeError):
        ops.nms(_nms_max_det_case().cuda(), 0, 0.25, 0.5, 30000, 1025)


def _iou32(a, b):
    """IoU of two xyxy fp32 boxes in the oracle's own arithmetic (nms_restated)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    area = lambda q: (q[2] - q[0]) * (q[3] - q[1])
    w = np.maximum(np.float32(0), np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]))
    h = np.maximum(np.float32(0), np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]))
    inter = w * h
    return np.float32(inter / (area(a) + area(b) - inter))


def _wh2xy(x):
    """xyxy rows of a [4+nc, N] input, as the oracle converts them (fp32)."""
    cx, cy, w, h = x[0], x[1], x[2], x[3]
    return torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).numpy()


def test_nms_iou_threshold_equality():
    """ovr > iou is strict: at iou == the pair's fp32 IoU both stay, one ulp lower the second goes."""
    x = torch.zeros(1, 5, 2)
    x[0, :, 0] = torch.tensor([50.3, 49.1, 41.7, 38.9, 0.9])
    x[0, :, 1] = torch.tensor([57.9, 52.6, 37.3, 43.1, 0.8])
    xy = _wh2xy(x[0])
    v = _iou32(xy[0], xy[1])
    assert 0.3 < v < 0.9
    below = np.nextafter(v, np.float32(0))
    ref_eq = _nms_check(x, 0.25, float(v))
    ref_lo = _nms_check(x, 0.25, float(below))
    assert len(ref_eq[0]) == 2 and len(ref_lo[0]) == 1


@pytest.mark.parametrize("nc", [1, 3])
def test_nms_conf_threshold_equality(nc):
    """score > conf is strict: a score equal to conf is no candidate, one ulp above is."""
    conf = 0.25
    above = float(np.nextafter(np.float32(conf), np.float32(1)))
    x = torch.zeros(1, 4 + nc, 3)
    x[0, 0] = torch.tensor([20.0, 200.0, 400.0])
    x[0, 1] = 30.0
    x[0, 2:4] = 10.0
    x[0, 4:] = 0.1
    x[0, 4 + nc - 1, 0] = conf
    x[0, 4, 1] = above
    x[0, 4 + nc - 1, 2] = float(np.nextafter(np.float32(conf), np.float32(0)))
    ref = _nms_check(x, conf, 0.5)
    assert len(ref[0]) == 1 and ref[0][0, 0].item() == 195.0 and ref[0][0, 4].item() == above


def test_nms_multilabel():
    """nc = 3: one box with two passing classes gives two rows; identical boxes of different
    classes never suppress each other; a NaN class score removes the whole box (amax propagates
    it); equal scores come out in a*nc + j order; +inf is a candidate and sorts first."""
    nan, inf = float("nan"), float("inf")
    boxes = torch.tensor([[100., 100., 40., 30.],     # 0: classes 0 and 2 pass
                          [100., 100., 40., 30.],     # 1: the same box, class 1
                          [300., 100., 40., 30.],     # 2: NaN in class 1 -> gone
                          [500., 100., 20., 20.],     # 3, 4: equal scores in several classes
                          [500., 300., 20., 20.],
                          [700., 300., 20., 20.],     # 5: +inf in class 1
                          [103., 101., 40., 30.]])    # 6: overlaps box 0 in class 0, lower score
    sc = torch.tensor([[0.9, 0.1, 0.8],
                       [0.1, 0.7, 0.1],
                       [0.95, nan, 0.95],
                       [0.5, 0.5, 0.1],
                       [0.5, 0.1, 0.5],
                       [0.1, inf, 0.1],
                       [0.6, 0.1, 0.1]])
    x = torch.cat([boxes, sc], 1).t().contiguous()[None]
    ref = _nms_check(x, 0.25, 0.5)[0]
    # (box, class) in output order: +inf first, then by score, ties by a*nc + j; box 6 suppressed
    exp = [(5, 1), (0, 0), (0, 2), (1, 1), (3, 0), (3, 1), (4, 0), (4, 2)]
    xy = torch.from_numpy(_wh2xy(x[0]))
    assert len(ref) == len(exp)
    for row, (a, j) in zip(ref, exp):
        assert torch.equal(row[:4], xy[a]) and row[4].item() == sc[a, j].item() and row[5].item() == j


def test_nms_degenerate_boxes_and_inf_score():
    """w = h = 0 twice at one place: IoU is 0/0 = NaN, NaN > iou is false, both are kept."""
    x = torch.zeros(1, 5, 4)
    x[0, :, 0] = torch.tensor([50., 60., 0., 0., 0.5])
    x[0, :, 1] = torch.tensor([50., 60., 0., 0., 0.6])
    x[0, :, 2] = torch.tensor([200., 60., 10., 10., float("inf")])
    x[0, :, 3] = torch.tensor([201., 60., 10., 10., 0.7])          # suppressed by the +inf box
    ref = _nms_check(x, 0.25, 0.5)[0]
    assert ref[:, 4].tolist() == torch.tensor([float("inf"), 0.6, 0.5]).tolist()


# ============================================================================= 2. metrics: update
def _rand_boxes(g, k, canvas=400.0, lo=5.0, span=80.0):
    c = torch.rand(k, 2, generator=g) * canvas
    return torch.cat([c, c + torch.rand(k, 2, generator=g) * span + lo], 1)


def _rand_dets(g, n, gt_i):
    """n prediction rows (xyxy, score, class 0): random boxes, every third one a jittered copy of
    one of the image's ground-truth boxes; scores quantised to 1/50, descending as NMS leaves them."""
    d = torch.zeros(n, 6)
    d[:, :4] = _rand_boxes(g, n)
    if len(gt_i) and n:
        idx = torch.arange(0, n, 3)
        pick = torch.randint(0, len(gt_i), (len(idx),), generator=g)
        d[idx, :4] = gt_i[pick] + (torch.rand(len(idx), 4, generator=g) - 0.5) * 6
    d[:, 4] = torch.sort(torch.round(torch.rand(n, generator=g) * 49 + 1) / 50, descending=True, stable=True)[0]
    return d


def _update_both(m, ref, dets, counts, gt, gidx):
    max_det = dets.shape[1]
    m.update_batch(dets.cuda(), counts.cuda(), gt.cuda(), gidx.cuda())
    ref.update_batch([dets[i, :min(int(counts[i]), max_det)] for i in range(len(counts))], gt, gidx)


def _check_state(m, ref):
    torch.cuda.synchronize()
    assert m.counters.cpu().tolist() == [ref.tp, ref.fp, ref.gt, len(ref.records)]
    n = min(len(ref.records), m.records.shape[0])
    exp = torch.tensor([[r[0], r[2]] for r in ref.records[:n]], dtype=torch.float64).reshape(n, 2).float()
    assert _same_bits(m.records[:n].cpu(), exp)


def _check_compute(m, ref, n):
    out, exp = m.compute(), ref.compute()
    tol = 1e-6 if n <= 2048 else 1e-5
    for k in ("precision", "recall", "f1"):
        assert out[k] == exp[k], (k, out[k], exp[k])
    for k in ("mAP50", "mAP75", "mAP"):
        assert abs(out[k] - exp[k]) <= tol * max(1.0, abs(exp[k])), (k, out[k], exp[k])
    return out, exp


def test_metrics_update_strided_prediction_loop():
    """counts 1024 / 321 / 320 at max_det = 1024: the 320-thread loop makes four trips, two
    (one of them a single prediction), and exactly one."""
    g = torch.Generator().manual_seed(3)
    B, max_det = 3, 1024
    counts = torch.tensor([1024, 321, 320], dtype=torch.int32)
    ng = [4, 3, 5]
    gts = [_rand_boxes(g, k) for k in ng]
    dets = torch.zeros(B, max_det, 6)
    for i in range(B):
        dets[i, :int(counts[i])] = _rand_dets(g, int(counts[i]), gts[i])
    m, ref = DetectionMetricsDevice("cuda", capacity=2048), R.DetectionMetricsRef()
    _update_both(m, ref, dets, counts, torch.cat(gts), torch.repeat_interleave(torch.arange(B), torch.tensor(ng)))
    _check_state(m, ref)
    assert len(ref.records) == 1665 and 0 < ref.tp < 1665
    _check_compute(m, ref, 1665)


def _mixed_batch(seed):
    """B = 6, max_det = 8, counts [5, 0, 7, 2000 (clamps to 8), 3, 0]; ground truth for images 0,
    1, 2 and 4 (image 1 has no prediction, image 3 no ground truth: both skipped, between used
    ones), rows shuffled so the images interleave, plus one row each with gt_batch -1 and B."""
    g = torch.Generator().manual_seed(seed)
    B, max_det = 6, 8
    counts = torch.tensor([5, 0, 7, 2000, 3, 0], dtype=torch.int32)
    ng = {0: 3, 1: 2, 2: 2, 4: 2}
    gts = {i: _rand_boxes(g, k) for i, k in ng.items()}
    dets = torch.zeros(B, max_det, 6)
    for i in range(B):                                # every row filled: rows past the count are not read
        dets[i] = _rand_dets(g, max_det, gts.get(i, []))
    gt = torch.cat([gts[i] for i in ng] + [_rand_boxes(g, 2)])
    gidx = torch.cat([torch.full((k,), i) for i, k in ng.items()] + [torch.tensor([-1, B])])
    perm = torch.randperm(len(gidx), generator=g)
    gt, gidx = gt[perm], gidx[perm]
    assert not bool((gidx[:-1] <= gidx[1:]).all())   # not in image order
    return dets, counts, gt, gidx


def test_metrics_update_mixed_counts_and_ground_truth():
    dets, counts, gt, gidx = _mixed_batch(11)
    m, ref = DetectionMetricsDevice("cuda", capacity=64), R.DetectionMetricsRef()
    _update_both(m, ref, dets, counts, gt, gidx)
    _check_state(m, ref)
    assert len(ref.records) == 5 + 7 + 3 and ref.gt == 3 + 2 + 2
    _check_compute(m, ref, len(ref.records))


def test_metrics_update_accumulates_and_skips_a_batch_without_ground_truth():
    m, ref = DetectionMetricsDevice("cuda", capacity=64), R.DetectionMetricsRef()
    _update_both(m, ref, *_mixed_batch(12))
    _check_state(m, ref)
    n1 = len(ref.records)
    dets, counts, _, _ = _mixed_batch(13)
    _update_both(m, ref, dets, counts, torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64))   # G = 0
    _check_state(m, ref)
    assert len(ref.records) == n1
    _update_both(m, ref, *_mixed_batch(14))
    _check_state(m, ref)
    assert len(ref.records) == 2 * n1
    _check_compute(m, ref, len(ref.records))


def test_metrics_update_nan_coordinate():
    """A NaN coordinate in a prediction box (image 0) and in one of three ground-truth boxes
    (image 1, where the row maximum must propagate it past a larger finite IoU): best IoU NaN,
    a false positive, the record NaN, and compute() as the oracle."""
    g = torch.Generator().manual_seed(17)
    gts = [_rand_boxes(g, 2), _rand_boxes(g, 3)]
    dets = torch.stack([_rand_dets(g, 6, gts[0]), _rand_dets(g, 6, gts[1])])
    dets[0, 3, 0] = float("nan")
    gts[1][1, 2] = float("nan")
    dets[1, 0, :4] = gts[1][2]                        # IoU 1 with the box after the NaN one
    dets[1, 1, :4] = gts[1][0]                        # IoU 1 with the box before it
    counts = torch.tensor([6, 6], dtype=torch.int32)
    m, ref = DetectionMetricsDevice("cuda", capacity=64), R.DetectionMetricsRef()
    _update_both(m, ref, dets, counts, torch.cat(gts), torch.tensor([0, 0, 1, 1, 1]))
    _check_state(m, ref)
    ious = [r[2] for r in ref.records]
    assert math.isnan(ious[3]) and all(math.isnan(v) for v in ious[6:]) and not any(r[1] for r in ref.records[6:])
    assert sum(math.isnan(v) for v in ious[:6]) == 1
    _check_compute(m, ref, 12)


def test_metrics_update_capacity():
    """14 records into a capacity of 10 over two calls: the count goes on, nothing is written past
    the records tensor (a slice of a larger sentinel-filled one), compute() refuses."""
    g = torch.Generator().manual_seed(19)
    sentinel = -12345.0
    big = torch.full((16, 2), sentinel, device="cuda")
    m, ref = DetectionMetricsDevice("cuda", capacity=1), R.DetectionMetricsRef()
    m.records = big[:10]
    for counts in ([5, 3], [4, 2]):
        gts = [_rand_boxes(g, 2), _rand_boxes(g, 1)]
        dets = torch.stack([_rand_dets(g, 8, gts[0]), _rand_dets(g, 8, gts[1])])
        _update_both(m, ref, dets, torch.tensor(counts, dtype=torch.int32), torch.cat(gts), torch.tensor([0, 0, 1]))
    _check_state(m, ref)                              # counters, and the first 10 records
    assert int(m.counters[3]) == 14 == len(ref.records)
    assert bool((big[10:] == sentinel).all())
    with pytest.raises(RuntimeError):
        m.compute()


# ============================================================================= 3. metrics: compute
def _compute_both(scores, ious, gt, label):
    """Write counters / records directly on both sides, compare the six outputs."""
    scores, ious = scores.float(), ious.float()
    n = len(scores)
    tp = int((ious > 0.5).sum())
    m = DetectionMetricsDevice("cuda", capacity=max(n, 1))
    m.counters.copy_(torch.tensor([tp, n - tp, gt, n]))
    m.records[:n] = torch.stack([scores, ious], 1).cuda()
    ref = R.DetectionMetricsRef()
    ref.tp, ref.fp, ref.gt = tp, n - tp, gt
    ref.records = [(s, v > 0.5, v) for s, v in zip(scores.tolist(), ious.tolist())]
    out, exp = m.compute(), ref.compute()
    d = max(abs(out[k] - exp[k]) for k in ("mAP50", "mAP75", "mAP"))
    print(f"det_metrics_compute {label}: n={n} max |AP diff| = {d:.3e}")
    tol = 1e-6 if n <= 2048 else 1e-5
    for k in ("precision", "recall", "f1"):
        assert out[k] == exp[k], (k, out[k], exp[k])
    for k in ("mAP50", "mAP75", "mAP"):
        assert abs(out[k] - exp[k]) <= tol * max(1.0, abs(exp[k])), (k, out[k], exp[k])
    return out, exp


def _q_scores(g, n):
    """positive scores quantised to 1/50: many ties"""
    return torch.round(torch.rand(n, generator=g) * 49 + 1) / 50


@pytest.mark.parametrize("n", [0, 1, 2, 2047, 2048, 2049, 4096, 4097])
def test_metrics_compute_tile_boundaries(n):
    g = torch.Generator().manual_seed(100 + n)
    ious = torch.rand(n, generator=g)
    # a false positive is kept only at IoU == 0.5 exactly (>= 0.5 but not > 0.5): without such
    # records every kept one is a TP and the fp prefix counts are never used
    ious[torch.rand(n, generator=g) < 0.3] = 0.5
    out, _ = _compute_both(_q_scores(g, n), ious, n // 2 + 3, "tiles")
    if n == 0:
        assert all(v == 0.0 for v in out.values())
    if n >= 2047:
        assert 0.0 < out["mAP50"] < 1.0 and 0.0 < out["mAP75"] < 1.0


@pytest.mark.parametrize("n", [300, 2049])
def test_metrics_compute_all_tp(n):
    g = torch.Generator().manual_seed(7)
    out, _ = _compute_both(_q_scores(g, n), torch.full((n,), 0.99), n + 10, "all-tp")
    assert out["precision"] > 0.999 and out["mAP50"] > 0.9 and abs(out["mAP"] - out["mAP50"]) < 1e-12


@pytest.mark.parametrize("n", [300, 2049])
def test_metrics_compute_all_fp_below_every_threshold(n):
    g = torch.Generator().manual_seed(8)
    out, exp = _compute_both(_q_scores(g, n), torch.full((n,), 0.3), n, "all-fp")
    assert out["mAP50"] == out["mAP75"] == out["mAP"] == 0.0 == exp["mAP"]


@pytest.mark.parametrize("n", [300, 2049])
def test_metrics_compute_kept_at_half_but_no_tp(n):
    """IoU exactly 0.5: kept at t = 0.5 (>=) but no true positive (> 0.5): AP50 exactly 0."""
    g = torch.Generator().manual_seed(9)
    out, exp = _compute_both(_q_scores(g, n), torch.full((n,), 0.5), n, "iou=0.5")
    assert out["mAP50"] == 0.0 == exp["mAP50"] and out["mAP"] == 0.0 and out["precision"] == 0.0


def test_metrics_compute_threshold_equality():
    """Records whose IoU is each of the ten fp32 thresholds exactly and one ulp below it."""
    g = torch.Generator().manual_seed(10)
    thr = torch.linspace(0.5, 0.95, 10)
    vals = torch.cat([thr, torch.nextafter(thr, torch.zeros(10))])
    ious = vals.repeat(12)[torch.randperm(240, generator=g)]
    out, _ = _compute_both(_q_scores(g, 240), ious, 200, "thr-eq")
    assert out["mAP75"] > 0.0


@pytest.mark.parametrize("low", [0.2, 0.5])
def test_metrics_compute_stable_order_one_score(low):
    """3000 records of one score, IoUs 0.9 / low alternating in blocks of 7 (coprime to the
    2048-record tile). With low = 0.5 the low records are kept false positives at t = 0.5, so
    AP50 depends on the insertion order alone, across the tile boundary: only a stable sort
    gives the oracle's answer. (With low = 0.2 they are kept nowhere.)"""
    n = 3000
    ious = torch.where((torch.arange(n) // 7) % 2 == 0, torch.tensor(0.9), torch.tensor(low))
    out, _ = _compute_both(torch.full((n,), 0.5), ious, 2000, f"stable-1 low={low}")
    if low == 0.5:
        # the reversed insertion order is another answer: the check means something
        rev = R.DetectionMetricsRef()
        rev.tp, rev.fp, rev.gt = int((ious > 0.5).sum()), int((ious <= 0.5).sum()), 2000
        rev.records = [(0.5, v > 0.5, v) for v in reversed(ious.tolist())]
        assert abs(rev.compute()["mAP50"] - out["mAP50"]) > 1e-4


def test_metrics_compute_stable_order_forty_scores():
    """40 distinct scores dealt round-robin over 4100 records, so every score group has records on
    both sides of insertion index 2048 and the sorted groups (102 or 103 long) straddle the sorted
    tile boundaries; the IoU (0.5 = a kept false positive) depends on the insertion index in
    blocks of 7."""
    n = 4100
    i = torch.arange(n)
    scores = (1 + i % 40).float() / 50
    ious = torch.tensor([0.9, 0.5, 0.6, 0.76, 0.5])[(i // 7) % 5]
    _compute_both(scores, ious, 3000, "stable-40")


def test_metrics_compute_after_reset_is_zero():
    g = torch.Generator().manual_seed(12)
    m = DetectionMetricsDevice("cuda", capacity=64)
    m.counters.copy_(torch.tensor([20, 20, 30, 40]))
    m.records[:40] = torch.stack([_q_scores(g, 40), torch.rand(40, generator=g)], 1).cuda()
    assert m.compute()["mAP50"] > 0.0
    m.reset()
    assert all(v == 0.0 for v in m.compute().values())


# ============================================================================= 4. eval loss
def _loss_margins(boxes, scores, gt, gidx, score_margin=True):
    """The reference-only input conditions: fp32 and fp64 take the same keep / positive decisions."""
    mx = scores.double().amax(1)
    if score_margin:
        assert bool(((mx - 0.01).abs() > 1e-5).all())
    for b in range(boxes.shape[0]):
        g = gt[gidx == b].double()
        keep = mx[b] > 0.01
        if len(g) and bool(keep.any()):
            best = R.compute_iou_ref(boxes[b].double().t()[keep], g).max(dim=1)[0]
            assert bool(((best - 0.5).abs() > 1e-4).all()), (b, float((best - 0.5).abs().min()))


def _loss_ref(boxes, scores, gt, gidx, labels, dtype=torch.float64):
    if labels is None:
        labels = torch.zeros(len(gidx), dtype=torch.int64)
    loss, per = R.detection_eval_loss_ref(boxes.to(dtype), scores.to(dtype), gt.to(dtype), labels, gidx)
    return float(loss), per


_LOSS_DIFF = {}


def _close(v, e, tol=2e-5):
    return (math.isnan(v) and math.isnan(e)) or abs(v - e) <= tol * max(1.0, abs(e))


def _loss_check(det, gt, gidx, labels, label, *, dtype=torch.float64, score_margin=True, pass_labels=True):
    """detection_eval_loss on det [B, 4+C, N] (any strides) against the reference; returns
    (device loss, device per_image, reference per-image dict)."""
    boxes, scores = det[:, :4], det[:, 4:]
    assert boxes.shape[2] != 4                         # the reference would take [B, 4, 4] as [B, N, 4]
    _loss_margins(boxes, scores, gt, gidx, score_margin)
    ref_loss, ref_per = _loss_ref(boxes, scores, gt, gidx, labels, dtype)
    loss, per = detection_eval_loss(det.cuda(), gt.cuda(), gidx.cuda(), labels.cuda() if pass_labels and labels is not None else None)
    torch.cuda.synchronize()
    loss, per = float(loss.cpu()), per.cpu().double()
    worst = 0.0
    for b in range(det.shape[0]):
        if b not in ref_per:
            assert per[b, 0].item() == 0.0, (b, per[b])
            continue
        for v, e in zip(per[b].tolist(), ref_per[b]):
            assert _close(v, e), (label, b, per[b].tolist(), ref_per[b])
            if not math.isnan(e):
                worst = max(worst, abs(v - e) / max(1.0, abs(e)))
    assert _close(loss, ref_loss), (label, loss, ref_loss)
    if not math.isnan(ref_loss):
        worst = max(worst, abs(loss - ref_loss) / max(1.0, abs(ref_loss)))
    _LOSS_DIFF[label] = worst
    print(f"det_eval_loss {label}: max scaled |diff| = {worst:.3e}")
    return loss, per, ref_per


@functools.lru_cache(maxsize=None)
def _loss_batch(C, seed=5):
    """B = 6, N = 64, one image per image-level branch (see the comments); gt rows interleaved."""
    g = torch.Generator().manual_seed(seed)
    B, N = 6, 64
    gtb = lambda k: _rand_boxes(g, k, lo=30.0)                       # sides 30..110
    far = lambda: _rand_boxes(g, N) + 2000.0                         # nowhere near any ground truth
    jit = lambda bx: bx + (torch.rand(bx.shape, generator=g) - 0.5) * 4
    boxes = torch.zeros(B, N, 4)
    scores = torch.rand(B, C, N, generator=g) * 0.009                # max <= 0.009: not kept

    def keep(b, idx):
        scores[b][:, idx] = torch.rand(C, len(idx), generator=g) * 3 + 0.05

    gts = {}
    boxes[0] = _rand_boxes(g, N); keep(0, torch.arange(0, N, 2))     # 0: no ground truth: skipped
    boxes[1] = _rand_boxes(g, N); gts[1] = gtb(3)                    # 1: ground truth, nothing kept (M = 0)
    boxes[2] = far(); keep(2, torch.arange(5, 40)); gts[2] = gtb(2)  # 2: kept, no positive (P = 0)
    gts[3] = gtb(4)                                                  # 3: positives and negatives
    boxes[3] = far()
    boxes[3, :12] = jit(gts[3][torch.arange(12) % 4])
    half = gts[3].clone()                                            # shifted by half a width: IoU ~ 1/3
    half[:, [0, 2]] += ((gts[3][:, 2] - gts[3][:, 0]) / 2)[:, None]
    boxes[3, 12:16] = half
    keep(3, torch.arange(0, 30))
    gts[4] = gtb(3)                                                  # 4: every kept prediction positive
    boxes[4] = far()
    boxes[4, 10:20] = jit(gts[4][torch.arange(10) % 3])
    keep(4, torch.arange(10, 20))
    gts[5] = torch.tensor([[10., 10., 50., 50.], [30., 10., 70., 50.]])   # 5: prediction 7 has IoU 0.6 with both
    boxes[5] = far()
    boxes[5, 7] = torch.tensor([20., 10., 60., 50.])
    boxes[5, 8:12] = jit(gts[5][[0, 1, 0, 1]])
    keep(5, torch.arange(0, 20))
    labels = {i: torch.randint(0, C, (len(v),), generator=g) for i, v in gts.items()}
    labels[5] = torch.tensor([1, 2]) % C                             # the tie is visible through cls
    gt = torch.cat([gts[i] for i in gts])
    gl = torch.cat([labels[i] for i in gts])
    gidx = torch.cat([torch.full((len(v),), i) for i, v in gts.items()])
    perm = torch.randperm(len(gidx), generator=g)
    gt, gl, gidx = gt[perm], gl[perm], gidx[perm]
    assert not bool((gidx[:-1] <= gidx[1:]).all())                   # interleaved
    det = torch.cat([boxes.transpose(1, 2), scores], 1).contiguous()
    # the tie really is one, in fp32 and in fp64
    for dt in (torch.float32, torch.float64):
        t = R.compute_iou_ref(boxes[5, 7:8].to(dt), gts[5].to(dt))[0]
        assert t[0].item() == t[1].item() and abs(t[0].item() - 0.6) < 1e-6
    return det, gt, gidx, gl


def _sub_batch(det, gt, gidx, gl, images):
    """the given images as a batch of their own"""
    sel = torch.cat([torch.nonzero(gidx == i).view(-1) for i in images]) if images else torch.zeros(0, dtype=torch.int64)
    sel = sel.sort()[0]
    remap = {i: k for k, i in enumerate(images)}
    return det[list(images)].contiguous(), gt[sel], torch.tensor([remap[int(i)] for i in gidx[sel]], dtype=torch.int64), gl[sel]


@pytest.mark.parametrize("C", [1, 3])
def test_eval_loss_every_image_level_branch(C):
    det, gt, gidx, gl = _loss_batch(C)
    loss, per, ref_per = _loss_check(det, gt, gidx, gl, f"branches C={C}")
    assert sorted(ref_per) == [2, 3, 4, 5]                        # 0 and 1 skipped
    assert math.isnan(ref_per[2][1]) and ref_per[2][0] == ref_per[2][3]        # P = 0: bg only
    assert all(math.isfinite(v) for v in ref_per[3]) and all(math.isfinite(v) for v in ref_per[5])
    assert math.isnan(ref_per[4][0]) and math.isnan(ref_per[4][3]) and math.isfinite(ref_per[4][1])
    assert math.isnan(loss)                                       # image 4 makes the batch loss NaN
    # ... so the other five as a batch of their own (finite loss), and image 4 alone
    loss5, _, _ = _loss_check(*_sub_batch(det, gt, gidx, gl, (0, 1, 2, 3, 5)), f"branches-without-4 C={C}")
    assert math.isfinite(loss5) and loss5 > 0.0
    loss1, per1, _ = _loss_check(*_sub_batch(det, gt, gidx, gl, (4,)), f"all-positive C={C}")
    assert math.isnan(loss1) and _same_bits(per1.float(), per[4:5].float())


def test_eval_loss_multiclass_labels_drive_the_cross_entropy():
    det, gt, gidx, gl = _sub_batch(*_loss_batch(3), (0, 1, 2, 3, 5))
    assert len(set(gl.tolist())) > 1
    _, per, _ = _loss_check(det, gt, gidx, gl, "C=3 labels")
    _, per0, _ = _loss_check(det, gt, gidx, torch.zeros_like(gl), "C=3 no labels", pass_labels=False)
    assert not torch.equal(per[:, 2], per0[:, 2])                 # the labels matter
    # prediction 7 of image 5 ties between two boxes with different labels; the reference takes
    # the first: with the pair's labels swapped cls changes, and still equals the reference
    img = 4                                                       # image 5 of the full batch
    rows = torch.nonzero(gidx == img).view(-1)
    swapped = gl.clone()
    swapped[rows] = gl[rows].flip(0)
    _, per_s, _ = _loss_check(det, gt, gidx, swapped, "C=3 tie labels swapped")
    assert per_s[img, 2].item() != per[img, 2].item()


@functools.lru_cache(maxsize=None)
def _loss_big(seed=23):
    """N = 1024 (the limit), B = 2, C = 2: about 600 kept predictions and 40 positives per image."""
    g = torch.Generator().manual_seed(seed)
    B, N, C = 2, 1024, 2
    boxes = torch.zeros(B, N, 4)
    scores = torch.rand(B, C, N, generator=g) * 0.009
    gts = []
    for b in range(B):
        gtb = _rand_boxes(g, 8, lo=30.0)
        gts.append(gtb)
        boxes[b] = _rand_boxes(g, N) + 2000.0
        perm = torch.randperm(N, generator=g)
        kept, pos = perm[:600 + b], perm[:40 + b]
        boxes[b, pos] = gtb[torch.arange(len(pos)) % 8] + (torch.rand(len(pos), 4, generator=g) - 0.5) * 4
        scores[b][:, kept] = torch.rand(C, len(kept), generator=g) * 3 + 0.05
    gt = torch.cat(gts)
    gidx = torch.repeat_interleave(torch.arange(B), 8)
    perm = torch.randperm(16, generator=g)
    det = torch.cat([boxes.transpose(1, 2), scores], 1).contiguous()
    return det, gt[perm], gidx[perm], torch.randint(0, C, (16,), generator=g)


def test_eval_loss_n_at_the_limit_strided_loops():
    det, gt, gidx, gl = _loss_big()
    kept = (det[:, 4:].amax(1) > 0.01).sum(1).tolist()
    assert kept == [600, 601]                                     # M > 256
    _, per, ref_per = _loss_check(det, gt, gidx, gl, "N=1024")
    assert all(all(math.isfinite(v) for v in ref_per[b]) for b in (0, 1))      # P*P = 1600 > 256


def test_eval_loss_n_limits():
    g = torch.Generator().manual_seed(29)
    gt = torch.tensor([[10., 10., 50., 60.]])
    gidx = torch.zeros(1, dtype=torch.int64)
    det = torch.tensor([[[11.], [10.], [50.], [61.], [0.9]]])     # N = 1: one positive, no negative
    loss, _, ref_per = _loss_check(det, gt, gidx, torch.zeros(1, dtype=torch.int64), "N=1")
    assert math.isnan(loss) and math.isfinite(ref_per[0][1])
    det = torch.tensor([[[311.], [10.], [350.], [61.], [0.9]]])   # N = 1: one negative
    loss, _, _ = _loss_check(det, gt, gidx, torch.zeros(1, dtype=torch.int64), "N=1 neg")
    assert math.isfinite(loss)
    big = torch.rand(1, 5, 1025, generator=g)
    with pytest.raises(PrpeError):
        detection_eval_loss(big.cuda(), gt.cuda(), gidx.cuda())


def test_eval_loss_strided_views_give_the_same_bits():
    det, gt, gidx, gl = _sub_batch(*_loss_batch(3), (0, 1, 2, 3, 5))
    B, ch, N = det.shape
    loss, per, _ = _loss_check(det, gt, gidx, gl, "view contiguous")
    nhwc = det.transpose(1, 2).contiguous().cuda()                # stored [B, N, 4+C]
    wide = torch.full((B, ch, 2 * N), 7.5).cuda()                 # every second column of [B, 4+C, 2N]
    wide[:, :, ::2] = det.cuda()
    for name, v in (("transposed", nhwc.transpose(1, 2)), ("every second column", wide[:, :, ::2])):
        assert not v.is_contiguous() and torch.equal(v.cpu(), det)
        l2, p2 = detection_eval_loss(v, gt.cuda(), gidx.cuda(), gl.cuda())
        torch.cuda.synchronize()
        assert _same_bits(p2.cpu(), per.float()) and float(l2.cpu()) == loss, name


def test_eval_loss_score_boundary_at_0_01():
    """max score == fp32(0.01) is not kept, one ulp above is: against the reference run in fp32."""
    edge = np.float32(0.01)
    above = np.nextafter(edge, np.float32(1))
    det = torch.zeros(1, 5, 6)
    det[0, :4] = (_rand_boxes(torch.Generator().manual_seed(1), 6) + 2000.0).t()
    det[0, :4, 5] = torch.tensor([11., 10., 50., 61.])            # one positive
    det[0, 4] = torch.tensor([float(edge), float(above), 2.0, 0.009, float(edge), 1.5])
    gt = torch.tensor([[10., 10., 50., 60.]])
    gidx = torch.zeros(1, dtype=torch.int64)
    _, per, ref_per = _loss_check(det, gt, gidx, torch.zeros(1, dtype=torch.int64), "score=0.01", dtype=torch.float32,
                                  score_margin=False)
    # the background mean is over exactly the two kept negatives (one ulp above 0.01, and 2.0)
    bce = lambda x: math.log1p(math.exp(x))
    assert abs(ref_per[0][3] - (bce(float(above)) + bce(2.0)) / 2) < 1e-6
