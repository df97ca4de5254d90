"""GPU: the stages around the models at every branch -- csrc/topdown.hip (crop_select,
crop_resize, crop_keypoints), csrc/ingest.hip (frame_ingest, crop_resize_u8) and csrc/poseeval.hip
(pose_eval_loss, OHKM, the COCO records) -- against the host restatements, which
tests/test_topdown_host.py, tests/test_ingest_host.py and tests/test_pose_eval_host.py pin to an
independent plain statement of each rule at the same edges.

Branch -> test (a parametrised case is named in brackets).

crop_select (``test_crop_select_edges``; inputs and literal expectations in
test_topdown_host.select_edge_cases):
* total > max_crops reached in a later 256-frame chunk [late_overflow]; counts < 0 at b >= 256
  [late_negative_count]; n == 0 [none]; n == max_crops [exactly_full]; counts > max_det, score ==
  thr / next float below / NaN score [prefix]; side == min_size / next float below [min_size];
  w > a h on both sides and at equality, with box_scale_x != box_scale_y [aspect]; +-inf
  coordinates and a window that overflows under pad, each using up a place [nonfinite].
crop_resize and crop_resize_u8 (every case runs through both):
* channels-last fp32 frames at a batch stride that is not C H W, source coordinates exactly on -1,
  W - 1, W (all four tap combinations), windows wholly under / over the clamp, w == 0, an empty
  slot in the middle, a frame index out of range: ``test_crop_resize_windows``.
* NaN and +-inf window fields: ``test_crop_resize_nonfinite_windows_give_zero_slots``.
* n_crops > max_crops, == 0, < 0: ``test_crop_resize_n_crops_out_of_range``.
* H == 1, W == 1, 1 x 1 and the thin 4 x 4096 frame: ``test_crop_resize_degenerate_frames``.
crop_keypoints: ``test_crop_keypoints_sizes`` (max_crops K below, at and above 256; n_crops >
  max_crops; n < n_crops < max_crops; coordinates outside [0, 1] and NaN).
frame_ingest: ``test_frame_ingest_edges`` (test_ingest_host.INGEST_EDGES: 1 x 1, Hs == 1, Ws == 1,
  nh == 1, nw == 1, 97 x 131 -> 3 x 5, an odd region off every edge, W < 256 with H % 8 == 0, and
  three identity cases), ``test_frame_ingest_y_amax`` (larger value kept, all-zero output, all
  negative, fill above every pixel, a stretch that must not see the fill).
pose_eval_loss: ``test_pose_eval_edges`` (test_pose_eval_host.POSE_EDGES: the REG boundary 4096 /
  4097, both in place; H W == 256, 35, 1; N = 64, 65, 256 with the only visibility 2 at n = 255;
  visibilities 0.5, 3, -1 and the skipped instance; the area and box clamps at 0.5 and 2, just
  inside, 0 and negative; a centre on a pixel, far outside, a tiny sigma; K = 1, 64; topk = 1, K;
  partner[k] == k in both modes; B = 9 with an all-zero frame; a NaN per-keypoint loss) and
  ``test_pose_eval_reg_boundary_pair_agrees``.
pose_coco_records: ``test_records_edges`` (K = 1, 5, 7, 64; a crowd instance between kept ones;
  masks that are no prefix; float32(0.3) against 0.3), ``test_records_capacity_and_counter``
  (capacity in the middle of an image, capacity 0, a counter and slot_base that are not 0).

Tolerances (none is taken from what the kernels give):
* crop_select: bit for bit against ``select_ref`` (fp32, contraction off), n_crops / status / row
  order against literals.
* crop_resize: the yardstick of tests/test_gpu_topdown.py (F.affine_grid + F.grid_sample in float64
  with the kernel's window, here for any frame size); e = its own noise when its grid is rounded
  to fp32, per group of windows; the kernel is allowed 4 e, e > 0 asserted. Exact zeros of the
  yardstick, empty slots, the border and channel 3 are exactly 0. crop_resize_u8 at a = 1, b = 0
  has the bits of crop_resize on u8.float().
* crop_keypoints: bit for bit against m2 + c * m4 in fp32 torch on the CPU (a product, then a
  sum); a NaN coordinate gives a NaN (its payload is not part of the contract).
* frame_ingest: 2^-14 raw units against ``ingest_ref`` in float64 (tests/test_gpu_ingest.py derives
  it: one ulp of [128, 256) per lerp stage and per rounded weight; coordinates are fp64, so it
  holds at any size); fill, border, channel 3 and y_amax exact; identity bit-equal.
* pose_eval_loss: the rules of tests/test_gpu_pose_eval.py, imported: target 4 ulps of the map's
  peak (band exemption capped at 0.1 %; the host file asserts that no pixel of any case is in
  the band), weights exact, avg and soft-argmax bit-identical, loss within max(4 e_ref, 16 ulp)
  of the fp64 restatement, ``check_loss_chain``.
* records: x, y bit-exact, v / bbox / area / indices exact, score 16 ulps (exact for K = 1).

Found by this file: ``pose_eval_kernel`` skipped an instance's keypoint with visibility <= 0
outright, where the reference multiplies its Gaussian by a mask of 0 -- and NaN * 0 is NaN, so
a processed instance with a negative area (NaN sigma) zeroes the thresholded map of EVERY
keypoint of the frame ([area_clamp], frame 5, keypoint 0). The kernel was wrong (the reference's
rule decides); it now carries such an instance as a masked one.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_ingest_host as I
import test_pose_eval_host as P
import test_topdown_host as T
from prpe import FrameIngest, ops
from prpe._lib import lib
from test_gpu_pose_eval import check_loss_chain, check_target, ulp32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH, CW = 256, 192
NAN, INF = float("nan"), float("inf")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _same_bits_or_both_nan(a, b):
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a)
    return a.shape == b.shape and torch.equal(nan, torch.isnan(b)) and torch.equal(_bits(a)[~nan], _bits(b)[~nan])


# ---------------------------------------------------------------------------------- crop_select
@pytest.mark.parametrize("name", sorted(T.select_edge_cases()))
def test_crop_select_edges(name):
    """Would catch: ``>=`` -> ``>`` at either threshold [prefix, min_size], ``>`` -> ``>=`` in the
    aspect test or sx / sy exchanged [aspect], the last finite test dropped [nonfinite], the
    max_det clamp dropped [prefix: frame 2 would take frame 3's rows], ``base_s`` not carried
    [late_overflow, late_negative_count: the second chunk would start at slot 0]."""
    dets, counts, kw, want_n, want_status, want_rows = T.select_edge_cases()[name]
    ref, n_ref, st_ref = T.select_ref(dets, counts, **kw)
    assert (n_ref, st_ref) == (want_n, want_status)
    max_crops = kw["max_crops"]
    meta = torch.full((max_crops, 8), 7.0, device=DEV)
    n = torch.full((1,), -9, device=DEV, dtype=torch.int32)
    st = torch.full((1,), -9, device=DEV, dtype=torch.int32)
    ops.crop_select(dets.to(DEV), counts.to(DEV), (64, 64), crop_meta=meta, n_crops=n, status=st,
                    **{k: v for k, v in kw.items() if k != "max_crops"})
    got = meta.cpu()
    assert (int(n), int(st)) == (want_n, want_status)
    assert T._frames_rows(got, want_n) == want_rows
    assert torch.equal(_bits(got), _bits(ref))


# ---------------------------------------------------------------------------------- crop_resize
def _yardstick(frames64, f, win, round_grid):
    """tests/test_gpu_topdown.py's yardstick for frames [B, 3, H, W] of any size."""
    H, W = frames64.shape[2:]
    x0, y0, w, h = (float(v) for v in win)
    theta = torch.tensor([[[w / W, 0.0, (2 * x0 + w) / W - 1.0], [0.0, h / H, (2 * y0 + h) / H - 1.0]]],
                         dtype=torch.float64)
    grid = F.affine_grid(theta, (1, 3, CH, CW), align_corners=False)
    if round_grid:
        grid = grid.float().double()
    return F.grid_sample(frames64[f:f + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]


def _source(B, H, W, seed, hi=256):
    """uint8 pixels in 1..255 (no zero inside a frame: an exact zero in a crop is an outside tap),
    as channels-last device tensors inside a 4-channel buffer: the fp32 view [B, 3, H, W] has
    sc == 1, sw == 4 and a batch stride of 4 H W; the uint8 view [B, H, W, 3] the same."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(1, hi, (B, H, W, 3), generator=g, dtype=torch.uint8)
    wide = torch.zeros(B, H, W, 4, dtype=torch.uint8)
    wide[..., :3] = u8
    wide_d = wide.to(DEV)
    f32 = wide_d.float()[..., :3].permute(0, 3, 1, 2)
    assert f32.stride(1) == 1 and f32.stride(0) == 4 * H * W != 3 * H * W
    return u8, wide_d[..., :3], f32


def _resize_both(u8_d, f32_d, meta, n_crops):
    """One crop_resize and one crop_resize_u8 launch into stale buffers; asserts the twin rule
    (same bits), the zero border and channel 3; returns the fp32 kernel's buffer on the host."""
    max_crops = meta.shape[0]
    n = torch.tensor([n_crops], device=DEV, dtype=torch.int32)
    bufs = []
    for _ in range(2):
        b = torch.zeros(max_crops, CH + 4, CW + 4, 4, device=DEV)
        b[:, 2:-2, 2:-2, :3] = 1.0                            # stale crops everywhere
        bufs.append(b)
    ops.crop_resize(f32_d, meta.to(DEV), n, bufs[0])
    ops.crop_resize_u8(u8_d, meta.to(DEV), n, bufs[1])
    a, b = bufs[0].cpu(), bufs[1].cpu()
    assert torch.equal(_bits(a), _bits(b))
    inner = torch.zeros_like(a, dtype=torch.bool)
    inner[:, 2:-2, 2:-2, :3] = True
    assert float(a[~inner].abs().max()) == 0.0
    return a


def _meta(rows, max_crops):
    meta = torch.zeros(max_crops, 8)
    ints = meta.view(torch.int32)
    ints[:, 0] = -1
    for s, (f, win) in enumerate(rows):
        ints[s, 0], ints[s, 1] = f, s
        meta[s, 2:6] = torch.tensor([float(v) for v in win], dtype=torch.float32)
        meta[s, 6] = 0.5
    return meta


def _check_against_yardstick(label, u8, wins, meta, buf, zero_slots=()):
    """4 e rule, exact zeros, and all-zero slots; returns the crops [slot, 3, 256, 192]."""
    frames64 = u8.permute(0, 3, 1, 2).double()
    live = [s for s, (f, _) in enumerate(wins) if 0 <= f < u8.shape[0] and s not in zero_slots]
    exact = {s: _yardstick(frames64, wins[s][0], meta[s, 2:6], False) for s in live}
    noise = max(float((_yardstick(frames64, wins[s][0], meta[s, 2:6], True) - exact[s]).abs().max()) for s in live)
    crops = buf[:, 2:-2, 2:-2, :3].permute(0, 3, 1, 2)
    errs = {s: float((crops[s].double() - exact[s]).abs().max()) for s in live}
    print(f"crop_resize {label}: yardstick fp32 noise e {noise:.3e}, bound 4 e {4 * noise:.3e}, kernel max|d| per "
          f"crop " + " ".join(f"[{s}] {e:.3e}" for s, e in errs.items()))
    assert noise > 0.0
    assert max(errs.values()) <= 4 * noise
    for s in live:
        assert _absmax(crops[s][exact[s] == 0]) == 0.0
    for s in range(buf.shape[0]):
        if s not in live:
            assert float(buf[s].abs().max()) == 0.0, s
    return crops, exact


H1, W1 = 40, 56


def test_crop_resize_windows():
    """Channels-last frames, the coordinates -1, W - 1 and W exactly, the clamps, w == 0, an empty
    slot and a frame index that is none, on both kernels. Slot 0's window (-1, -1, 192, 256) puts
    source coordinate j - 1 on output column j with weight 0: the crop is the frame shifted by
    one pixel, bit for bit, and exactly 0 outside it -- column 0 (xa = -1 out, xb = 0 in), column
    56 (xa = 55 in, xb = 56 out) and column 57 (both out), rows likewise. Would catch: ``ina``
    and ``inb`` exchanged, ``<`` -> ``<=`` in a bounds test, the wrong stride for a channel."""
    u8, u8_d, f32_d = _source(3, H1, W1, 71)
    wins = [(1, (-1.0, -1.0, 192.0, 256.0)),                  # integer coordinates -1 .. 190 / -1 .. 254
            (0, (-500.0, 5.0, 100.0, 20.0)),                  # every column under the -2 clamp
            (-1, (0.0, 0.0, 0.0, 0.0)),                       # an empty slot in the middle
            (0, (5.0, 500.0, 20.0, 100.0)),                   # every row over the H + 1 clamp
            (2, (20.25, 4.0, 0.0, 30.0)),                     # w == 0: one source column
            (7, T.window_ref(20, 8, 34, 26, 1.25)),           # a frame index out of range
            (2, (-1.5, -1.5, 60.0, 44.0)),                    # crosses all four edges off the pixel grid
            (0, (5.0, -500.0, 20.0, 100.0)), (0, (500.0, 5.0, 100.0, 20.0))]   # under in y, over in x
    meta = _meta(wins, len(wins) + 1)
    buf = _resize_both(u8_d, f32_d, meta, len(wins))
    crops, exact = _check_against_yardstick("40x56 channels-last", u8, wins, meta, buf)
    for s in (1, 3, 7, 8):                                    # wholly outside: the yardstick's zeros, exactly
        assert float(exact[s].abs().max()) == 0.0 and float(crops[s].abs().max()) == 0.0
    want = torch.zeros(3, CH, CW)
    want[:, 1:H1 + 1, 1:W1 + 1] = u8[1].permute(2, 0, 1).float()
    assert torch.equal(crops[0], want)
    assert float(crops[0][:, 1:H1 + 1, 1:W1 + 1].min()) >= 1.0       # an exact zero beside a non-zero
    assert bool((crops[4] == crops[4][:, :, :1]).all()) and float(crops[4].max()) > 100.0
    assert float(crops[6].max()) > 100.0


def test_crop_resize_nonfinite_windows_give_zero_slots():
    """NaN and +-inf window fields (the file's comment: "NaN -> -2"): a slot of zeros, the border
    untouched, the finite slot beside them still right.

    Every address formed is in bounds, read from the code before this was run: the frame index
    passes ``(unsigned)f < (unsigned)B`` first. ``sx`` leaves ``fmin(fmax(., -2.0), W + 1.0)``:
    fmax of a NaN and -2.0 is -2.0, of -inf is -2.0, and +inf is cut to W + 1 by fmin, so the
    clamped value is a finite number in [-2, W + 1] BEFORE ``floor`` and the ``(int)`` conversion;
    xa is in [-2, W + 1] and xb in [-1, W + 2]. Either is used in an address only as ``ina ? xa :
    0``, i.e. after ``(unsigned)xa < (unsigned)W``, so the column offset is in [0, W - 1]; rows
    the same with H; the channel offset is c * sc with c in 0..2. Outputs are addressed by slot,
    row and thread index alone. A non-finite x field makes every column tap an outside one
    (v00 .. v11 = 0, so the lerps give 0 whatever ay is); a non-finite y field every row tap."""
    u8, u8_d, f32_d = _source(2, H1, W1, 72)
    good = (10.0, 5.0, 30.0, 28.0)
    bad = [(NAN, 5.0, 30.0, 28.0), (10.0, NAN, 30.0, 28.0), (10.0, 5.0, NAN, 28.0), (10.0, 5.0, 30.0, NAN),
           (INF, 5.0, 30.0, 28.0), (-INF, 5.0, 30.0, 28.0), (10.0, INF, 30.0, 28.0), (10.0, -INF, 30.0, 28.0),
           (10.0, 5.0, INF, 28.0), (10.0, 5.0, -INF, 28.0), (10.0, 5.0, 30.0, INF), (10.0, 5.0, 30.0, -INF),
           (-INF, 5.0, INF, 28.0), (NAN, NAN, NAN, NAN)]
    wins = [(0, good)] + [(1, w) for w in bad] + [(1, good)]
    meta = _meta(wins, len(wins))
    buf = _resize_both(u8_d, f32_d, meta, len(wins))
    zero = tuple(range(1, len(bad) + 1))
    crops, _ = _check_against_yardstick("non-finite windows", u8, wins, meta, buf, zero_slots=zero)
    for s in zero:
        assert float(buf[s].abs().max()) == 0.0, wins[s]
    assert float(crops[0].min()) >= 1.0 and float(crops[-1].min()) >= 1.0


@pytest.mark.parametrize("n_crops,filled", [(100, 2), (0, 0), (-3, 0), (1, 1)])
def test_crop_resize_n_crops_out_of_range(n_crops, filled):
    """n_crops above max_crops counts as max_crops, 0 and a negative count as none (would catch a
    missing clamp, or ``slot < n`` compared unsigned)."""
    u8, u8_d, f32_d = _source(1, 12, 16, 73)
    wins = [(0, (2.0, 1.0, 9.0, 8.0)), (0, (0.0, 0.0, 16.0, 12.0))]
    buf = _resize_both(u8_d, f32_d, _meta(wins, 2), n_crops)
    for s in range(2):
        inner = buf[s, 2:-2, 2:-2, :3]
        assert (float(inner.max()) > 1.0) if s < filled else (float(buf[s].abs().max()) == 0.0)


@pytest.mark.parametrize("B,H,W,wins", [
    (2, 1, 9, [(0, (0.0, 0.0, 9.0, 1.0)), (1, (-2.0, -1.5, 12.0, 4.0)), (1, (3.25, 0.0, 2.5, 1.0))]),
    (2, 7, 1, [(0, (0.0, 0.0, 1.0, 7.0)), (1, (-1.5, -2.0, 4.0, 12.0)), (1, (0.0, 2.25, 1.0, 2.5))]),
    (1, 1, 1, [(0, (0.0, 0.0, 0.75, 1.0)), (0, (-1.0, -1.0, 3.0, 4.0)), (0, (0.25, 0.25, 0.75, 1.0))]),
    (1, 4, 4096, [(0, (4000.0, -1.0, 90.0, 6.0)), (0, (4080.5, 0.5, 20.0, 3.0)), (0, (1.0, 0.0, 3.0, 4.0))]),
], ids=["H1", "W1", "1x1", "thin_4x4096"])
def test_crop_resize_degenerate_frames(B, H, W, wins):
    """Single-pixel sides (every second tap is outside) and a long thin frame with windows at its
    far end: the coordinates are formed in fp64, so the kernel's error stays under the
    yardstick's own fp32 noise there (which grows with W). Would catch a coordinate formed in
    fp32, or ``(unsigned)yb < H`` tested against W.

    On the 1 x 1 frame the yardstick's noise is below fp32's own output rounding whatever the
    window (a grid error of 2^-24 moves the sample by 2^-25 of a pixel there, and the only
    contrast is the pixel against the zeros around it), so 4 e can only be met where the kernel's
    arithmetic is exact: the pixel values are below 16 and the windows step by 1 / 256 and 1 / 64
    of a pixel from dyadic origins, so every weight has at most 9 bits, every product and sum
    fits fp32, and any distance from the yardstick beyond its own fp64 rounding is a wrong tap
    or weight."""
    u8, u8_d, f32_d = _source(B, H, W, 74 + H, hi=16 if (H, W) == (1, 1) else 256)
    meta = _meta(wins, len(wins) + 1)
    buf = _resize_both(u8_d, f32_d, meta, len(wins))
    crops, exact = _check_against_yardstick(f"{H}x{W}", u8, wins, meta, buf)
    for s in range(len(wins)):
        assert float(crops[s].max()) >= 1.0                   # the crop holds the image


# ---------------------------------------------------------------------------------- crop_keypoints
@pytest.mark.parametrize("K,max_crops,n,n_crops", [(1, 5, 5, 3), (64, 4, 4, 4), (133, 3, 3, 2), (17, 4, 4, 9),
                                                   (17, 6, 2, 4), (5, 3, 3, 0), (5, 3, 3, -2)])
def test_crop_keypoints_sizes(K, max_crops, n, n_crops):
    """max_crops K = 5, 256 and 399 threads' worth; slots at or past min(n_crops, n, max_crops)
    are exactly 0 in a buffer of ones (would catch ``t >= total`` -> ``>``, the clamp to
    max_crops or to n dropped, a fused multiply-add: one rounding instead of two)."""
    g = torch.Generator().manual_seed(80 + K)
    wins = [(s % 2, T.window_ref(20.3 + s, 8.1, 54.7 + 3 * s, 46.9 + s, 1.25)) for s in range(max_crops)]
    meta = _meta(wins, max_crops)
    coords = torch.rand(n, K, 2, generator=g) * 3.0 - 1.0     # outside [0, 1] too
    coords[0, 0, 0], coords[n - 1, K - 1, 1] = NAN, NAN
    scores = torch.rand(n, K, generator=g)
    kp = torch.ones(max_crops, K, 3, device=DEV)
    ops.crop_keypoints(coords.to(DEV), scores.to(DEV), meta.to(DEV),
                       torch.tensor([n_crops], device=DEV, dtype=torch.int32), kp)
    live = max(min(n_crops, n, max_crops), 0)
    want = torch.zeros(max_crops, K, 3)
    want[:live, :, 0] = meta[:live, 2:3] + coords[:live, :, 0] * meta[:live, 4:5]
    want[:live, :, 1] = meta[:live, 3:4] + coords[:live, :, 1] * meta[:live, 5:6]
    want[:live, :, 2] = scores[:live]
    got = kp.cpu()
    assert _same_bits_or_both_nan(got, want)
    assert _absmax(got[live:]) == 0.0
    if live:
        assert bool(torch.isnan(got[0, 0, 0])) and float(got[0, :, 2].max()) > 0.0
        assert bool((coords[:live] < 0).any()) and bool((coords[:live] > 1).any())


def test_crop_keypoints_refuses_more_rows_than_slots():
    meta = _meta([(0, (0.0, 0.0, 10.0, 10.0))], 2).to(DEV)
    n = torch.ones(1, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match="3 crops of keypoints for a list of 2 slots"):
        ops.crop_keypoints(torch.zeros(3, 4, 2, device=DEV), torch.zeros(3, 4, device=DEV), meta, n,
                           torch.zeros(2, 4, 3, device=DEV))


# ---------------------------------------------------------------------------------- frame_ingest
BOUND = 2.0 ** -14
AB = ((0.0123, -0.5, 1 / 255), (-1.5, 3.25, 0.1))


def _ingest(u8, size, region, ing, amax0=None):
    """prpe_frame_ingest into the interior of a zero-bordered [B, H + 6, W + 8, 4] buffer with a
    stale interior; (buffer, y_amax) on the host."""
    B = u8.shape[0]
    H, W = size
    buf = torch.zeros(B, H + 6, W + 8, 4, device=DEV)
    buf[:, 3:3 + H, 3:3 + W, :] = -3.0
    amax = (torch.zeros(B) if amax0 is None else amax0.clone()).to(DEV)
    ops.frame_ingest(u8.to(DEV), buf[:, 3:3 + H, 3:3 + W, :], region, ing.a, ing.b, ing.fill, ing.swap_rb,
                     y_amax=amax)
    buf = buf.cpu()
    inner = torch.zeros_like(buf, dtype=torch.bool)
    inner[:, 3:3 + H, 3:3 + W, :3] = True
    assert float(buf[~inner].abs().max()) == 0.0              # border and channel 3
    return buf[:, 3:3 + H, 3:3 + W, :3], amax.cpu()


@pytest.mark.parametrize("name", sorted(I.INGEST_EDGES))
def test_frame_ingest_edges(name):
    """Would catch: ``xa + 1 < Ws`` -> ``<=`` (a read past a one-pixel side; in bounds of the
    tensor only by luck), ``top`` / ``left`` exchanged [odd_region_off_every_edge], ``rows``
    mis-sized when H % 8 == 0 [narrow_with_whole_row_groups]."""
    (Hs, Ws), size, region = I.INGEST_EDGES[name]
    identity = name.startswith("identity")
    u8 = I.edge_source(name)
    ing = FrameIngest(size=size, mode="stretch", norm=AB if identity else I.RAW, fill=(114, 3, 250))
    got, amax = _ingest(u8, size, region, ing)
    ref = I.ingest_ref(u8, ing, region=region)
    top, left, nh, nw = region
    inside = torch.zeros(size, dtype=torch.bool)
    inside[top:top + nh, left:left + nw] = True
    a, b = torch.tensor(ing.a), torch.tensor(ing.b)
    if identity:
        assert torch.equal(_bits(got[:, top:top + nh, left:left + nw]), _bits(u8.float() * a + b))
    else:
        err = float((got.double() - ref).abs().max())
        print(f"frame_ingest {name} {Hs}x{Ws} -> {size} region {region}: max|d| {err:.3e}, bound {BOUND:.3e}")
        assert err <= BOUND
        assert float(ref[:, inside].max()) > 150.0            # not vacuous
    fill = torch.tensor(ing.fill) * a + b
    outside = got[:, ~inside]
    assert torch.equal(_bits(outside), _bits(fill.expand_as(outside)))
    assert torch.equal(_bits(amax), _bits(got.abs().flatten(1).max(1)[0]))


@pytest.mark.parametrize("case", ["larger_kept", "all_zero", "all_negative", "fill_above_pixels", "stretch_no_fill"])
def test_frame_ingest_y_amax(case):
    """The y_amax contract: slot = max(slot, max|y|) from the kernel's own output and the slot's
    previous content. Would catch: the ``m > 0`` guard turned into a store [all_zero: the slot
    keeps 0.25], ``fabsf`` dropped [all_negative], ``om = 0.f`` dropped inside the region
    [stretch_no_fill: the fill's 255 would show], ``om = fmx`` dropped [fill_above_pixels]."""
    g = torch.Generator().manual_seed(90)
    u8 = torch.randint(1, 101, (2, 10, 14, 3), generator=g, dtype=torch.uint8)      # pixels 1 .. 100
    size, prev, norm, fill, mode = (16, 24), torch.zeros(2), I.RAW, 255, "letterbox"
    if case == "larger_kept":
        prev = torch.tensor([1000.0, 0.5])
    elif case == "all_zero":
        norm, fill, prev = ((0, 0, 0), (0, 0, 0)), 0, torch.tensor([0.0, 0.25])
    elif case == "all_negative":
        norm = ((-1.0, -2.0, -0.5), (-3.0, -1.0, -7.0))
    elif case == "stretch_no_fill":
        mode = "stretch"
    ing = FrameIngest(size=size, mode=mode, norm=norm, fill=fill)
    region = ing.geometry(10, 14)
    got, amax = _ingest(u8, size, region, ing, amax0=prev)
    want = torch.maximum(prev, got.abs().flatten(1).max(1)[0])
    assert torch.equal(_bits(amax), _bits(want))
    if case == "larger_kept":
        assert amax.tolist()[0] == 1000.0 and amax.tolist()[1] == 255.0
    elif case == "all_zero":
        assert amax.tolist() == [0.0, 0.25] and float(got.abs().max()) == 0.0
    elif case == "all_negative":
        assert float(got.max()) < 0.0 and float(amax.min()) > 100.0
    elif case == "fill_above_pixels":
        assert region != (0, 0, 16, 24) and amax.tolist() == [255.0, 255.0]
    else:
        assert region == (0, 0, 16, 24) and float(amax.max()) <= 100.0 and float(amax.min()) > 50.0


# ---------------------------------------------------------------------------------- pose_eval_loss
def _run_pose(c, inplace):
    K = c["heat"].shape[1]
    part = [-1] * K
    for a, b in c["pairs"]:
        part[a], part[b] = b, a
    h = c["heat"].to(DEV)
    out = ops.pose_eval_loss(h, c["kp"].to(DEV), c["kpw"], heat_flipped=c["heat_f"].to(DEV), partner=part,
                             mode=0 if c["mode"] == "reference" else 1,
                             areas=None if c["areas"] is None else c["areas"].to(DEV), boxes=c["boxes"].to(DEV),
                             sigma=c["sigma"], topk=c["topk"], avg_out=h if inplace else None, want_avg=True,
                             want_argmax=True, want_target=True)
    if inplace:
        assert out["avg"].data_ptr() == h.data_ptr()
    return {k: v.cpu() for k, v in out.items()}, part


def _restate(c):
    H, W = c["heat"].shape[2:]
    avg = P.ref_flip_average(c["heat"], c["heat_f"], c["mode"], c["pairs"])
    target, weights = P.ref_target(c["kp"], c["areas"], H, W, c["sigma"])
    pre = P.ref_target(c["kp"], c["areas"], H, W, c["sigma"], thresholded=False)[0]
    t64, w64 = P.ref_target(c["kp"], c["areas"], H, W, c["sigma"], torch.float64)
    l32 = P.ref_loss(avg, target, weights, c["kpw"], c["topk"])
    l64 = P.ref_loss(P.ref_flip_average(c["heat"].double(), c["heat_f"].double(), c["mode"], c["pairs"]), t64, w64,
                     c["kpw"], c["topk"])
    return avg, target, weights, pre, l32, l64


@pytest.mark.parametrize("name", P.POSE_EDGES)
def test_pose_eval_edges(name):
    """The rules of tests/test_gpu_pose_eval.py on every edge case. Would catch: ``HW <= 4096`` ->
    ``<`` [reg_4096 would re-read; in place it still must give the same bits], ``tid < p.N`` ->
    ``lane < p.N`` or rw[3] left out of the weight's maximum [n_256: weight 1 comes from instance
    255 alone], ``vis == 2.f`` -> ``>= 2.f`` [visibility: 3 weighs 0.5], ``if (any)`` dropped
    [visibility: frame 1's weights are 0], ``w < 0.5f`` -> ``<=`` is invisible but ``/ 96`` ->
    ``/ 95`` is not [area_clamp], ``rank < topk`` -> ``<=`` [topk_1, k_1], a wave that stops after
    its first frame [ohkm_9_frames]. [area_clamp] is the case the kernel fix of the module
    docstring answers (read from the earlier kernel's code: frame 5's keypoint 0 kept the other
    instance's Gaussian there)."""
    c = P.pose_edge_case(name)
    B, K, H, W = c["heat"].shape
    out, part = _run_pose(c, inplace=name.startswith("reg_"))
    avg, target, weights, pre, (l32, pk32), (l64, pk64) = _restate(c)
    assert torch.equal(out["avg"], avg)
    assert torch.equal(out["weights"], weights)
    assert not bool(torch.isnan(out["target"]).any())
    check_target(out["target"], target, torch.nan_to_num(pre, nan=0.0))
    nan_maps = torch.isnan(pre).flatten(2).any(2)
    assert not bool(out["target"][nan_maps].any()) and not bool(target[nan_maps].any())
    # soft-argmax: the unfused kernel on the same average, bit for bit, and the restatement
    c_u, s_u, am_u = ops.softargmax(avg.to(DEV), c["boxes"][:, 0].to(DEV), want_argmax=True)
    assert torch.equal(out["coords"], c_u.cpu()) and _same_bits_or_both_nan(out["scores"], s_u)
    assert torch.equal(out["argmax"], am_u.cpu())
    rc, rs = P.ref_keypoints(avg, c["boxes"][:, 0])
    torch.testing.assert_close(out["coords"], rc, rtol=0, atol=1e-6)
    torch.testing.assert_close(out["scores"], rs, rtol=1e-5, atol=1e-7, equal_nan=True)
    assert torch.equal(out["argmax"].long(), avg.reshape(B, K, -1).argmax(dim=2))
    # the loss
    got = float(out["loss"][0])
    if name == "ohkm_nan":
        # by NaN-ness, and by value elsewhere: the chain's 1-ulp rule on the columns that are numbers
        assert torch.equal(torch.isnan(out["per_kp"]), torch.isnan(pk32)) and bool(torch.isnan(pk32[:, 3]).all())
        top = torch.topk(out["per_kp"], c["topk"], dim=1)[0].sum()
        assert bool(torch.isnan(top)) and got != got and bool(torch.isnan(l32)) and bool(torch.isnan(l64))
        keep = [k for k in range(K) if k != 3]
        sub = {k: (v[:, keep] if k in ("avg", "target", "weights", "per_kp") else v) for k, v in out.items()}
        sub["loss"] = (torch.topk(sub["per_kp"].double(), c["topk"], dim=1)[0].sum() / (B * c["topk"])).float().view(1)
        check_loss_chain(sub, c["topk"], [c["kpw"][k] for k in keep])
        print(f"pose_eval {name}: loss NaN as torch.topk gives; per_kp NaN in column 3 only")
        return
    e_ref, d = abs(float(l32) - float(l64)), abs(got - float(l64))
    bound = max(4 * e_ref, 16 * ulp32(float(l64)))
    print(f"pose_eval {name} {tuple(c['kp'].shape[:3])} {H}x{W}: loss gpu {got:.9g} fp64 {float(l64):.12g} "
          f"e_ref {e_ref:.3g} bound {bound:.3g} distance {d:.3g}")
    assert d <= bound
    check_loss_chain(out, c["topk"], c["kpw"])
    # literal expectations that only the exercised branch produces
    if name == "n_256":
        assert float(out["weights"][0, 2]) == 1.0 and float(out["weights"][0, 0]) == 0.5
    if name == "visibility":
        assert out["weights"].tolist() == [[0.5, 0.5, 0.5, 1.0], [0.0] * 4, [0.5, 1.0, 0.5, 1.0]]
        assert not bool(out["target"][1].any()) and not bool(out["target"][0, 2].any())
    if name == "area_clamp":
        assert not bool(out["target"][5].any()) and all(bool(out["target"][b].any()) for b in (0, 1, 2, 3, 4, 6))
        assert bool(torch.isnan(out["scores"][5]).all()) and not bool(torch.isnan(out["scores"][[0, 1, 2, 3, 4, 6]]).any())
    if name == "tiny_sigma":
        assert float(out["target"][0, 0, 2, 3]) == 1.0 and int((out["target"] != 0).sum()) == 1
    if name == "centres":
        assert not bool(out["target"][0, 1].any()) and int(out["target"][0, 0].argmax()) == 2 * W + 3
    if name == "ohkm_9_frames":
        assert not bool(out["per_kp"][4].any()) and bool(out["per_kp"][[0, 8]].all())
    if name == "map_1x1":
        assert out["argmax"].tolist() == [[0] * K] * B and bool((out["coords"] == 0.5).all())


def test_pose_eval_reg_boundary_pair_agrees():
    """4096 pixels (registers) against 4097 (re-reading), same streams: frame 0's keypoint 0 has a
    zero target, weight 0.5 and the same 4096 predictions (+ one 0) in both, so H W per_kp[0, 0] is
    the same sum of squares; each side is within the chain's 1 ulp of it, so they differ by at
    most the two ulps together."""
    vals = {}
    for name in ("reg_4096", "reg_4097"):
        c = P.pose_edge_case(name)
        out, _ = _run_pose(c, inplace=True)
        HW = c["heat"].shape[2] * c["heat"].shape[3]
        assert float(out["weights"][0, 0]) == 0.5 and not bool(out["target"][0, 0].any())
        exact = float((out["avg"][0, 0].double() ** 2).sum()) * 0.5 * float(np.float32(c["kpw"][0]))
        vals[name] = float(out["per_kp"][0, 0]) * HW
        assert abs(vals[name] - exact) <= HW * ulp32(exact / HW)
    a, b = vals["reg_4096"], vals["reg_4097"]
    print(f"pose_eval REG pair: H W per_kp[0, 0] = {a:.9g} (4096) and {b:.9g} (4097), |d| {abs(a - b):.3g}")
    assert a > 0 and abs(a - b) <= 4096 * ulp32(a / 4096) + 4097 * ulp32(b / 4097)


# ---------------------------------------------------------------------------------- pose_coco_records
SENT = -7.0


def _records(c, capacity, counter0=0, slot_base=0, rows=16):
    """prpe_pose_coco_records into sentinel-filled buffers of ``rows`` records with the given
    ``capacity`` (<= rows, so writes past it would show); (counter, kpts, meta) on the host."""
    K = c["coords"].shape[1]
    B, N = c["masks"].shape
    dev = [c[k].to(DEV).contiguous() for k in ("coords", "scores", "boxes", "areas")]
    mk, cr = c["masks"].to(torch.uint8).to(DEV), c["crowd"].to(torch.uint8).to(DEV)
    keep = (C.c_uint8 * B)(*c["keep"])
    counter = torch.tensor([counter0], dtype=torch.int64, device=DEV)
    kpts, meta = torch.full((rows, K, 3), SENT, device=DEV), torch.full((rows, 8), SENT, device=DEV)
    assert 0 <= capacity <= rows
    rc = lib().prpe_pose_coco_records(*[t.data_ptr() for t in dev], mk.data_ptr(), cr.data_ptr(),
                                      C.cast(keep, C.c_void_p), B, N, K, c["thresh"], slot_base, counter.data_ptr(),
                                      kpts.data_ptr(), meta.data_ptr(), capacity, None)
    assert rc == 0
    torch.cuda.synchronize()
    return int(counter.item()), kpts.cpu().numpy(), meta.cpu().numpy()


def _check_records(c, got, first, written, slot_base):
    """Records [first, first + written) equal the restatement's first ``written``; all others
    keep the sentinel."""
    _, kpts, meta = got
    rk, rm = P.ref_records(c["coords"].numpy(), c["scores"].numpy(), c["boxes"], c["areas"], c["masks"], c["crowd"],
                           c["keep"], c["thresh"], slot_base=slot_base)
    K = rk.shape[1]
    sl = slice(first, first + written)
    assert np.array_equal(kpts[sl].view(np.int32), rk[:written].view(np.int32))          # x, y bit-exact, v exact
    assert np.array_equal(meta[sl, :2].view(np.int32), rm[:written, :2].view(np.int32))  # image and instance index
    assert np.array_equal(meta[sl, 3:], rm[:written, 3:])                                # bbox, area
    if K == 1:
        assert np.array_equal(meta[sl, 2], rm[:written, 2])
    else:
        np.testing.assert_allclose(meta[sl, 2], rm[:written, 2], rtol=16 * 2.0 ** -24, atol=0)
    rest = np.ones(len(kpts), dtype=bool)
    rest[sl] = False
    assert (kpts[rest] == SENT).all() and (meta[rest] == SENT).all()
    return rk, rm


@pytest.mark.parametrize("name", ["k_1", "k_5", "k_7", "k_64"])
def test_records_edges(name):
    """Would catch: ``lane < 8`` tied to ``has_k`` [k_1, k_7: the meta row would be short],
    ``lim`` counted from the masked positions instead of ``masks.sum()`` [image 0 gives instances
    0 and 1, image 2 gives 1 and 2], a crowd instance taking a slot, ``(double)sc > thresh``
    compared in float [float32(0.3) would give v = 1]."""
    c = P.records_edge_case(name)
    got = _records(c, 16)
    rk, rm = _check_records(c, got, 0, 7, 0)
    assert got[0] == 7 == len(rk)
    order = [tuple(int(v) for v in row) for row in got[2][:7, :2].copy().view(np.int32)]
    assert order == c["want_order"]
    assert got[1][0, 0, 2] == 2.0 and (rk.shape[1] == 1 or got[1][0, 1, 2] == 1.0)


@pytest.mark.parametrize("capacity,counter0,slot_base,first,written",
                         [(4, 0, 0, 0, 4), (0, 0, 0, 0, 0), (16, 3, 40, 3, 7), (6, 3, 40, 3, 3), (2, 3, 0, 0, 0)])
def test_records_capacity_and_counter(capacity, counter0, slot_base, first, written):
    """capacity 4 falls inside image 1's three records (slots 2, 3, 4): slot 3 is written, slot 4
    is not, though the buffer has room; the counter still counts all 7. capacity 0 writes nothing.
    A starting counter of 3 with slot_base 40 appends at slot 3 with image indices 40 .. 42 (would
    catch ``r < cap`` -> ``<=``, the counter advanced by the written records only, ``before``
    added without the counter)."""
    c = P.records_edge_case("k_5")
    got = _records(c, capacity, counter0, slot_base)
    assert got[0] == counter0 + 7
    _, rm = _check_records(c, got, first, written, slot_base)
    if written:
        assert int(got[2][first, :1].copy().view(np.int32)[0]) == slot_base
