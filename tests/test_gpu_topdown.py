"""GPU: top-down pose (csrc/topdown.hip, prpe.topdown) -- the crop list against the torch
restatement of tests/test_topdown_host.py, the resample against torch's own CPU grid_sample, the
keypoint map, and TopDownPose against the unfused route through the public pieces.

Tolerances (none is taken from what the kernels give):
* crop_select: integer fields, window and score bit-exact (fp32, contraction off).
* crop_resize: the yardstick is F.affine_grid + F.grid_sample(bilinear, zeros, align_corners=False)
  in float64 on the CPU with the kernel's window. Its own fp32 noise e = max |yardstick -
  yardstick with its grid rounded to fp32| on these inputs; the kernel is allowed 4 e. Border,
  channel 3 and empty slots exactly zero; a constant frame gives the constant exactly wherever
  the four taps are inside the frame.
* crop_keypoints: bit-exact against x0 + cx * w in fp32.
* TopDownPose: bit-identical keypoints to the unfused route and between compact modes.
"""
import pytest
import torch
import torch.nn.functional as F

import test_topdown_host as T
from prpe import CombinedModel, TopDownPose, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH, CW = 256, 192


def _alloc(max_crops):
    return (torch.empty(max_crops, 8, device=DEV), torch.empty(1, device=DEV, dtype=torch.int32),
            torch.empty(1, device=DEV, dtype=torch.int32))


def _meta_from_windows(rows, max_crops):
    """[(frame, (x0, y0, w, h)), ...] -> crop_meta [max_crops, 8] (host) as crop_select lays it out."""
    meta = torch.zeros(max_crops, 8)
    ints = meta.view(torch.int32)
    ints[:, 0] = -1
    for s, (f, win) in enumerate(rows):
        ints[s, 0], ints[s, 1] = f, s
        meta[s, 2:6] = torch.stack([torch.as_tensor(v, dtype=torch.float32) for v in win])
        meta[s, 6] = 0.5
    return meta


# ---------------------------------------------------------------------------------- crop_select
def test_crop_select_matches_the_restatement_bit_for_bit():
    g = torch.Generator().manual_seed(5)
    B, max_det = 5, 8
    xy = torch.rand(B, max_det, 2, generator=g) * 100
    wh = torch.rand(B, max_det, 2, generator=g) * 60 + 10.0
    score = torch.sort(torch.rand(B, max_det, generator=g) * 0.7 + 0.3, dim=1, descending=True)[0]
    dets = torch.cat([xy, xy + wh, score[..., None], torch.zeros(B, max_det, 1)], 2)
    dets[3, 1, 0] = float("nan")                      # skipped, and uses up one of frame 3's two
    counts = torch.tensor([3, 0, -1, 7, 1], dtype=torch.int32)
    kw = dict(score_thr=0.25, max_per_frame=2, min_size=4.0, box_scale=(1.7, 2.3), pad=1.25)
    for max_crops, want_n, want_status in ((4, 4, 1), (3, 3, 3), (9, 4, 1)):
        ref, n_ref, st_ref = T.select_ref(dets, counts, max_crops=max_crops, **kw)
        assert (n_ref, st_ref) == (want_n, want_status)
        meta, n, st = _alloc(max_crops)
        meta.fill_(7.0)
        ops.crop_select(dets.to(DEV), counts.to(DEV), (240, 320), crop_meta=meta, n_crops=n, status=st, **kw)
        assert int(n) == n_ref and int(st) == st_ref
        assert torch.equal(meta.cpu().view(torch.int32), ref.view(torch.int32))
    assert T._frames_rows(ref, n_ref) == [(0, 0), (0, 1), (3, 0), (4, 0)]


def test_crop_select_scans_more_frames_than_threads():
    """B > 256: the scan runs in chunks of 256 frames with a carried base."""
    B = 600
    g = torch.Generator().manual_seed(6)
    xy = torch.rand(B, 3, 2, generator=g) * 50
    dets = torch.cat([xy, xy + 20 + torch.rand(B, 3, 2, generator=g), torch.full((B, 3, 1), 0.5),
                      torch.zeros(B, 3, 1)], 2)
    counts = torch.randint(0, 4, (B,), generator=g).int()
    ref, n_ref, st_ref = T.select_ref(dets, counts, max_per_frame=3, max_crops=1000)
    meta, n, st = _alloc(1000)
    ops.crop_select(dets.to(DEV), counts.to(DEV), (64, 64), crop_meta=meta, n_crops=n, status=st, max_per_frame=3)
    assert int(n) == n_ref == int(counts.sum()) and int(st) == st_ref == 0
    assert torch.equal(meta.cpu().view(torch.int32), ref.view(torch.int32))


# ---------------------------------------------------------------------------------- crop_resize
H, W = 40, 56
CONST = 0.7


def _yardstick(frames64, f, win, round_grid):
    x0, y0, w, h = (float(v) for v in win)
    theta = torch.tensor([[[w / W, 0.0, (2 * x0 + w) / W - 1.0], [0.0, h / H, (2 * y0 + h) / H - 1.0]]],
                         dtype=torch.float64)
    grid = F.affine_grid(theta, (1, 3, CH, CW), align_corners=False)
    if round_grid:
        grid = grid.float().double()
    return F.grid_sample(frames64[f:f + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]


@pytest.fixture(scope="module")
def resized():
    """One launch on all the boxes, shared by the crop_resize tests."""
    g = torch.Generator().manual_seed(7)
    big = torch.rand(3, 3, 48, 64, generator=g)
    big[2] = CONST
    big_d = big.to(DEV)
    frames = big_d[:, :, 4:4 + H, 5:5 + W]                    # a non-contiguous slice
    assert not frames.is_contiguous()
    wins = [(0, T.window_ref(20, 8, 34, 26, 1.25)),           # wholly inside
            (1, T.window_ref(2, 1, 54, 39, 1.25)),            # crosses all four frame edges
            (0, T.window_ref(-30, -20, 90, 70, 1.25)),        # larger than the frame
            (1, T.window_ref(30, 20, 34, 24, 1.25)),          # 4 x 4 pixels: heavy magnification
            (0, (0.0, 0.0, float(W), float(H))),              # exactly the frame
            (2, T.window_ref(20, 8, 34, 26, 1.25)),           # constant frame, inside
            (2, T.window_ref(2, 1, 54, 39, 1.25))]            # constant frame, crossing the edges
    max_crops = len(wins) + 2
    meta = _meta_from_windows(wins, max_crops)
    buf = torch.zeros(max_crops, CH + 4, CW + 4, 4, device=DEV)
    buf[:, 2:-2, 2:-2, :3] = 1.0                              # stale crops everywhere
    n = torch.tensor([len(wins)], device=DEV, dtype=torch.int32)
    ops.crop_resize(frames, meta.to(DEV), n, buf)
    return big[:, :, 4:4 + H, 5:5 + W].double(), wins, meta, buf.cpu()


def test_crop_resize_against_cpu_grid_sample(resized):
    frames64, wins, meta, buf = resized
    exact = [_yardstick(frames64, f, meta[s, 2:6], False) for s, (f, _) in enumerate(wins)]
    noise = max(float((_yardstick(frames64, f, meta[s, 2:6], True) - exact[s]).abs().max())
                for s, (f, _) in enumerate(wins))
    errs = [float((buf[s, 2:-2, 2:-2, :3].permute(2, 0, 1).double() - exact[s]).abs().max())
            for s in range(len(wins))]
    print(f"crop_resize: yardstick fp32 noise {noise:.3e}, bound {4 * noise:.3e}, kernel max|d| per crop "
          + " ".join(f"{e:.3e}" for e in errs))
    assert 0.0 < noise < 1e-4
    assert max(errs) <= 4 * noise
    for s in range(len(wins)):                                # not vacuous: the crops hold the image
        assert float(exact[s].abs().max()) > 0.2


def test_crop_resize_keeps_border_and_clears_empty_slots(resized):
    _, wins, _, buf = resized
    inner = torch.zeros_like(buf, dtype=torch.bool)
    inner[:, 2:-2, 2:-2, :3] = True
    assert float(buf[~inner].abs().max()) == 0.0              # border and channel 3 of every slot
    assert float(buf[len(wins):].abs().max()) == 0.0          # slots at or past n_crops: the ones are gone
    assert float(buf[:len(wins)].abs().max()) > 0.0


def test_crop_resize_constant_frame_is_exact(resized):
    _, wins, meta, buf = resized
    for s, (f, _) in enumerate(wins):
        if f != 2:
            continue
        x0, y0, w, h = (meta[s, c].double() for c in (2, 3, 4, 5))
        sx = x0 + (torch.arange(CW, dtype=torch.float64) + 0.5) * (w / CW) - 0.5
        sy = y0 + (torch.arange(CH, dtype=torch.float64) + 0.5) * (h / CH) - 0.5
        in_x = (sx.floor() >= 0) & (sx.floor() + 1 <= W - 1)
        in_y = (sy.floor() >= 0) & (sy.floor() + 1 <= H - 1)
        inside = in_y[:, None] & in_x[None, :]
        assert int(inside.sum()) > 1000
        got = buf[s, 2:-2, 2:-2, :3]
        assert bool((got[inside] == torch.tensor(CONST)).all())
        if not bool(inside.all()):
            assert float(got[~inside].max()) <= float(torch.tensor(CONST))


def test_crop_resize_refuses_a_short_buffer():
    meta, n, _ = _alloc(4)
    frames = torch.zeros(1, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="crops"):
        ops.crop_resize(frames, meta, n, torch.zeros(3, CH + 4, CW + 4, 4, device=DEV))
    with pytest.raises(ValueError, match="crops"):
        ops.crop_resize(frames, meta, n, torch.zeros(4, CH + 4, CW + 4, 8, device=DEV)[..., :4])
    with pytest.raises(ValueError, match="kpts"):
        ops.crop_keypoints(torch.zeros(2, 17, 2, device=DEV), torch.zeros(2, 17, device=DEV), meta, n,
                           torch.zeros(3, 17, 3, device=DEV))


# ---------------------------------------------------------------------------------- crop_keypoints
def test_crop_keypoints_bit_exact_and_empty_slots_zero():
    g = torch.Generator().manual_seed(8)
    wins = [(0, T.window_ref(20.3, 8.1, 34.7, 26.9, 1.25)), (1, T.window_ref(2.2, 1.1, 54.4, 39.3, 1.25)),
            (1, T.window_ref(-30.5, -20.25, 90.125, 70.7, 1.25))]
    meta = _meta_from_windows(wins, 5)
    coords, scores = torch.rand(4, 17, 2, generator=g), torch.rand(4, 17, generator=g)
    kp = torch.ones(5, 17, 3, device=DEV)
    n = torch.tensor([3], device=DEV, dtype=torch.int32)
    ops.crop_keypoints(coords.to(DEV), scores.to(DEV), meta.to(DEV), n, kp)
    want = torch.zeros(5, 17, 3)
    want[:3, :, 0] = meta[:3, 2:3] + coords[:3, :, 0] * meta[:3, 4:5]
    want[:3, :, 1] = meta[:3, 3:4] + coords[:3, :, 1] * meta[:3, 5:6]
    want[:3, :, 2] = scores[:3]
    assert torch.equal(kp.cpu().view(torch.int32), want.view(torch.int32))
    n.fill_(5)                                        # the pose net ran on 4 slots only: slot 4 stays empty
    ops.crop_keypoints(coords.to(DEV), scores.to(DEV), meta.to(DEV), n, kp)
    assert float(kp[4].abs().max()) == 0.0 and float(kp[3, :, 2].max()) > 0.0


# ---------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model(state_dict):
    return CombinedModel(state_dict, device=DEV)


def _hand_dets():
    dets = torch.zeros(2, 4, 6)
    dets[0, 0, :5] = torch.tensor([100.0, 60.0, 300.0, 560.0, 0.9])
    dets[0, 1, :5] = torch.tensor([400.0, 300.0, 700.0, 620.0, 0.8])      # leaves the frame
    dets[1, 0, :5] = torch.tensor([250.5, 120.25, 380.0, 330.0, 0.7])
    return dets.to(DEV), torch.tensor([2, 1], device=DEV, dtype=torch.int32)


def test_topdown_equals_the_unfused_route(model):
    frames = synth.frames(2).to(DEV)
    dets, counts = _hand_dets()
    kw = dict(max_per_frame=2, max_crops=4, box_scale=1.0)
    out = TopDownPose(model, compact=False, **kw).from_detections(frames, dets, counts)
    n = int(out["n_crops"])
    assert n == 3 and int(out["status"]) == 0
    meta = out["crop_meta"]
    ref, n_ref, _ = T.select_ref(dets, counts.cpu(), max_per_frame=2, max_crops=4)
    assert torch.equal(meta.cpu().view(torch.int32), ref.view(torch.int32))
    # the unfused route: the kernel's crops read back, then the public pieces
    crops = model.engine.crop_pix4(4)[:n, 2:-2, 2:-2, :3].permute(0, 3, 1, 2).contiguous()
    assert float(crops.abs().max()) > 0.5
    heat = model.vitpose_from_pixels(crops).heatmaps
    coords, scores = ops.softargmax(heat)
    want = torch.stack([meta[:n, 2:3] + coords[..., 0] * meta[:n, 4:5],
                        meta[:n, 3:4] + coords[..., 1] * meta[:n, 5:6], scores], 2)
    kp = out["keypoints"].clone()
    assert torch.equal(kp[:n].view(torch.int32), want.view(torch.int32))
    assert float(kp[n:].abs().max()) == 0.0 and bool(torch.isfinite(kp).all())
    # compact: ViTPose on the first n slots only, same bits
    out_c = TopDownPose(model, compact=True, **kw).from_detections(frames, dets, counts)
    assert torch.equal(out_c["keypoints"].view(torch.int32), kp.view(torch.int32))
    # fewer crops in the next call: nothing stale in the keypoints or in the crop buffer
    counts2 = torch.tensor([1, 0], device=DEV, dtype=torch.int32)
    for compact in (False, True):
        out2 = TopDownPose(model, compact=compact, **kw).from_detections(frames, dets, counts2)
        assert int(out2["n_crops"]) == 1
        assert torch.equal(out2["keypoints"][:1].view(torch.int32), kp[:1].view(torch.int32))
        assert float(out2["keypoints"][1:].abs().max()) == 0.0
        assert float(model.engine.crop_pix4(4)[1:].abs().max()) == 0.0
    people = TopDownPose.results(out)
    assert [len(p) for p in people] == [2, 1] and torch.equal(people[1][0]["keypoints"], kp[2].cpu())


def test_topdown_full_path(model):
    frames = synth.frames(2).to(DEV)
    stride = model.yolo_person.yolo.head.stride
    model.yolo_person.yolo.head.stride = torch.tensor([8.0, 16.0, 32.0])
    try:
        out = TopDownPose(model, score_thr=0.0)(frames)
    finally:
        model.yolo_person.yolo.head.stride = stride
    assert out["dets"].shape == (2, 300, 6) and out["counts"].shape == (2,)
    assert out["crop_meta"].shape == (16, 8) and out["keypoints"].shape == (16, 17, 3)
    assert out["n_crops"].shape == (1,) and out["status"].shape == (1,)
    counts = out["counts"].cpu()
    assert bool((counts >= 0).all())
    assert int(out["n_crops"]) == min(int(counts.clamp(max=8).sum()), 16)
    assert bool(torch.isfinite(out["keypoints"]).all())
