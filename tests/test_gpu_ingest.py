"""GPU: uint8 frames in (csrc/ingest.hip, prpe.ingest) -- prpe_frame_ingest against the torch
restatement of tests/test_ingest_host.py, prpe_crop_resize_u8 against prpe_crop_resize, and the
uint8 entry points of CombinedModel and TopDownPose against their float routes.

Tolerances (none is taken from what the kernels give):
* identity (region = source size): bit-equal to torch's u8.float() * a + b (an fp32 multiply, then
  an fp32 add); channel 3, the border, fill pixels and y_amax exact.
* resample: the yardstick is ``ingest_ref`` in float64 on the CPU; the bound is 2^-14 raw units =
  4 ulp of values in [128, 256): one per lerp stage for its two roundings (the horizontal pair
  enters the vertical lerp with weights summing to 1) and one per rounded weight at |delta| <= 255.
* crop_resize_u8: bit-identical to crop_resize on the float copy of the frames (a = 1, b = 0), and
  to that result * a + b in filled slots.
* model / top-down: bit-identical to the float routes.
Measured on the MI355X (max |kernel - float64 yardstick|, raw units, bound 6.10e-05): 37x53 ->
32x48 stretch 2.04e-05, -> 32x48 letterbox 2.52e-05, -> 48x32 letterbox 1.39e-05; 10x14 -> 2.04e-05,
2.37e-05, 1.59e-05; 7x9 -> 11x523 3.13e-05.
"""
import pytest
import torch

import test_ingest_host as I
import test_topdown_host as T
from prpe import CombinedModel, FrameIngest, TopDownPose, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2.0 ** -14


def _run(u8_dev, ingest, want_amax=True, stale=0.0):
    """prpe_frame_ingest into the interior of a stem-shaped buffer [B, H+6, W+8, 4] (border zero,
    interior ``stale``); (buffer on the host, y_amax on the host)."""
    B, Hs, Ws, _ = u8_dev.shape
    H, W = ingest.size
    buf = torch.zeros(B, H + 6, W + 8, 4, device=DEV)
    buf[:, 3:3 + H, 3:3 + W, :] = stale
    amax = torch.zeros(B, device=DEV) if want_amax else None
    ops.frame_ingest(u8_dev, buf[:, 3:3 + H, 3:3 + W, :], ingest.geometry(Hs, Ws), ingest.a, ingest.b, ingest.fill,
                     ingest.swap_rb, y_amax=amax)
    return buf.cpu(), (amax.cpu() if want_amax else None)


def _border_and_c3_zero(buf, H, W):
    inner = torch.zeros_like(buf, dtype=torch.bool)
    inner[:, 3:3 + H, 3:3 + W, :3] = True
    return float(buf[~inner].abs().max()) == 0.0


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------- 1. identity
AB = ((0.0123, -0.5, 1 / 255), (-1.5, 3.25, 0.1))


def _identity_frames():
    g = torch.Generator().manual_seed(21)
    u8 = torch.randint(0, 256, (2, 24, 40, 3), generator=g, dtype=torch.uint8)
    u8[1] //= 4                                       # other magnitudes: a slot mix-up shows in y_amax
    return u8


@pytest.mark.parametrize("source", ["hwc", "bgr", "nchw_permuted", "w_slice"])
def test_identity_is_bit_exact(source):
    u8 = _identity_frames()
    ing = FrameIngest(size=(24, 40), mode="stretch", norm=AB, channel_order="bgr" if source == "bgr" else "rgb")
    if source == "nchw_permuted":
        src = u8.permute(0, 3, 1, 2).contiguous().to(DEV).permute(0, 2, 3, 1)
        assert src.stride(3) == 24 * 40
    elif source == "w_slice":
        wide = torch.full((2, 24, 50, 3), 255, dtype=torch.uint8)
        wide[:, :, 5:45] = u8
        src = wide.to(DEV)[:, :, 5:45]
        assert not src.is_contiguous()
    else:
        src = u8.to(DEV)
    buf, amax = _run(src, ing, stale=7.0)
    x = u8.flip(3) if source == "bgr" else u8
    want = x.float() * torch.tensor(ing.a) + torch.tensor(ing.b)
    assert buf.shape == (2, 30, 48, 4)
    assert torch.equal(_bits(buf[:, 3:27, 3:43, :3]), _bits(want))
    assert _border_and_c3_zero(buf, 24, 40)
    want_amax = want.abs().flatten(1).max(1)[0]
    assert float(want_amax[0]) != float(want_amax[1])
    assert torch.equal(_bits(amax), _bits(want_amax))


# ---------------------------------------------------------------------------------- 2. resample
@pytest.fixture(scope="module")
def sources():
    g = torch.Generator().manual_seed(22)
    return {"down": torch.randint(0, 256, (3, 37, 53, 3), generator=g, dtype=torch.uint8),
            "up": torch.randint(0, 256, (2, 10, 14, 3), generator=g, dtype=torch.uint8)}


@pytest.mark.parametrize("which", ["down", "up"])
@pytest.mark.parametrize("size,mode", [((32, 48), "stretch"), ((32, 48), "letterbox"), ((48, 32), "letterbox")])
def test_resample_within_the_derived_bound(sources, which, size, mode):
    u8 = sources[which]
    ing = FrameIngest(size=size, mode=mode, norm=I.RAW)
    H, W = size
    top, left, nh, nw = ing.geometry(*u8.shape[1:3])
    assert (mode == "stretch") == ((nh, nw) == (H, W))
    buf, amax = _run(u8.to(DEV), ing, stale=-3.0)
    got = buf[:, 3:3 + H, 3:3 + W, :3]
    ref = I.ingest_ref(u8, ing)                       # float64
    err = float((got.double() - ref).abs().max())
    print(f"frame_ingest {which} {tuple(u8.shape[1:3])} -> {size} {mode}: max|d| {err:.3e}, bound {BOUND:.3e}")
    assert err <= BOUND
    assert float(ref.abs().max()) > 200.0             # not vacuous
    region = torch.zeros(H, W, dtype=torch.bool)
    region[top:top + nh, left:left + nw] = True
    fill = torch.tensor(ing.fill) * torch.tensor(ing.a) + torch.tensor(ing.b)
    outside = got[:, ~region]
    assert torch.equal(_bits(outside), _bits(fill.expand_as(outside)))
    assert _border_and_c3_zero(buf, H, W)
    assert torch.equal(_bits(amax), _bits(got.abs().flatten(1).max(1)[0]))


# ---------------------------------------------------------------------------------- 3. launch shape
def test_launch_shape_wide_rows_and_a_ragged_row_count():
    """W = 523: a thread walks three columns (stride 256) and the last pass is partial; H = 11: the
    second workgroup of a frame holds 3 of its 8 rows."""
    g = torch.Generator().manual_seed(23)
    u8 = torch.randint(0, 256, (3, 7, 9, 3), generator=g, dtype=torch.uint8)
    u8[1] //= 3
    u8[2] //= 9
    ing = FrameIngest(size=(11, 523), mode="stretch", norm=I.RAW)
    buf, amax = _run(u8.to(DEV), ing, stale=300.0)
    got = buf[:, 3:14, 3:526, :3]
    err = float((got.double() - I.ingest_ref(u8, ing)).abs().max())
    print(f"frame_ingest (7, 9) -> (11, 523): max|d| {err:.3e}, bound {BOUND:.3e}")
    assert err <= BOUND
    assert _border_and_c3_zero(buf, 11, 523)
    own = got.abs().flatten(1).max(1)[0]
    assert torch.equal(_bits(amax), _bits(own)) and float(own[0]) > float(own[1]) > float(own[2]) > 0.0


# ---------------------------------------------------------------------------------- 4. crop_resize_u8
H4, W4 = 40, 56


def _meta(rows, max_crops):
    meta = torch.zeros(max_crops, 8)
    ints = meta.view(torch.int32)
    ints[:, 0] = -1
    for s, (f, win) in enumerate(rows):
        ints[s, 0], ints[s, 1] = f, s
        meta[s, 2:6] = torch.stack([torch.as_tensor(v, dtype=torch.float32) for v in win])
        meta[s, 6] = 0.5
    return meta


@pytest.fixture(scope="module")
def crops():
    """The frames (quantised) and windows of tests/test_gpu_topdown.py's resample test, plus an
    empty slot inside the list and a frame index out of range; one reference launch, shared."""
    g = torch.Generator().manual_seed(7)
    big = (torch.rand(3, 3, 48, 64, generator=g) * 255).round().to(torch.uint8)
    big[2] = 179
    big_d = big.to(DEV)
    u8 = big_d[:, :, 4:4 + H4, 5:5 + W4].permute(0, 2, 3, 1)       # NCHW slice seen as NHWC
    assert not u8.is_contiguous()
    wins = [(0, T.window_ref(20, 8, 34, 26, 1.25)),           # wholly inside
            (1, T.window_ref(2, 1, 54, 39, 1.25)),            # crosses all four frame edges
            (0, T.window_ref(-30, -20, 90, 70, 1.25)),        # larger than the frame
            (-1, (0.0, 0.0, 0.0, 0.0)),                       # an empty slot
            (1, T.window_ref(30, 20, 34, 24, 1.25)),          # 4 x 4 pixels: heavy magnification
            (0, (0.0, 0.0, float(W4), float(H4))),            # exactly the frame
            (7, T.window_ref(20, 8, 34, 26, 1.25)),           # a frame index out of range
            (2, T.window_ref(2, 1, 54, 39, 1.25))]            # constant frame, crossing the edges
    max_crops = len(wins) + 2
    meta = _meta(wins, max_crops).to(DEV)
    n = torch.tensor([len(wins)], device=DEV, dtype=torch.int32)
    ref = torch.zeros(max_crops, 260, 196, 4, device=DEV)
    ref[:, 2:-2, 2:-2, :3] = 1.0
    ops.crop_resize(big_d[:, :, 4:4 + H4, 5:5 + W4].float(), meta, n, ref)
    filled = torch.tensor([0 <= f < 3 for f, _ in wins] + [False, False])
    return u8, meta, n, ref.cpu(), filled


def _crop_u8(u8, meta, n, **kw):
    buf = torch.zeros(meta.shape[0], 260, 196, 4, device=DEV)
    buf[:, 2:-2, 2:-2, :3] = 1.0                              # stale crops everywhere
    ops.crop_resize_u8(u8, meta, n, buf, **kw)
    return buf.cpu()


def test_crop_resize_u8_has_the_bits_of_crop_resize(crops):
    u8, meta, n, ref, filled = crops
    got = _crop_u8(u8, meta, n)
    assert torch.equal(_bits(got), _bits(ref))
    assert float(ref[filled].abs().max()) > 100.0 and float(ref[~filled].abs().max()) == 0.0
    # bgr on channel-flipped frames: the same crops
    assert torch.equal(_bits(_crop_u8(u8.flip(3), meta, n, swap_rb=True)), _bits(ref))


def test_crop_resize_u8_normalises_filled_slots_only(crops):
    u8, meta, n, ref, filled = crops
    ing = FrameIngest(norm="imagenet")
    got = _crop_u8(u8, meta, n, a=ing.a, b=ing.b)
    want = torch.zeros_like(ref)
    want[filled, 2:-2, 2:-2, :3] = (ref[filled, 2:-2, 2:-2, :3] * torch.tensor(ing.a) + torch.tensor(ing.b))
    assert torch.equal(_bits(got), _bits(want))
    # taps outside the frame contribute raw 0, so a pixel wholly outside is b exactly
    assert float(got[2, 2, 2, 0]) == ing.b[0]
    inner = torch.zeros_like(got, dtype=torch.bool)
    inner[:, 2:-2, 2:-2, :3] = True
    assert float(got[~inner].abs().max()) == 0.0 and float(got[~filled].abs().max()) == 0.0


# ---------------------------------------------------------------------------------- 5. end to end
@pytest.fixture(scope="module")
def model(state_dict):
    return CombinedModel(state_dict, device=DEV)


STRIDE = [8.0, 16.0, 32.0]


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def test_forward_u8_equals_forward_on_the_float_frames(model):
    g = torch.Generator().manual_seed(24)
    u8 = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8)
    ing = FrameIngest(size=(64, 64), mode="stretch", norm="unit")
    x = (u8.permute(0, 3, 1, 2).float() * torch.tensor(ing.a).view(1, 3, 1, 1)
         + torch.tensor(ing.b).view(1, 3, 1, 1)).to(DEV)
    u8_d = u8.to(DEV)
    for concurrent in (True, False):
        want = model.forward_all(x, face_stride=STRIDE, concurrent=concurrent)
        got = model.forward_all_u8(u8_d, ing, face_stride=STRIDE, concurrent=concurrent)
        assert set(got) == set(want) == {"det", "emb", "norm", "heatmaps"}
        for k in want:
            assert _same(got[k], want[k]), (k, concurrent)
        assert float(want["heatmaps"].abs().max()) > 0.0
    task0 = model.current_task
    try:
        for task in CombinedModel.SUPPORTED_TASKS:
            model.set_task(task)
            want, got = model(x), model.forward_u8(u8_d, ing)
            if task == "pose_estimation":
                assert _same(got.heatmaps, want.heatmaps)
            elif task == "face_recognition":
                assert _same(got[0], want[0]) and _same(got[1], want[1])
            else:
                assert _same(got, want)
    finally:
        model.set_task(task0)
    with pytest.raises(ValueError, match="float32"):
        model(u8_d.permute(0, 3, 1, 2))                       # uint8 into forward still raises


def test_forward_all_u8_letterbox_differs_from_the_float_route_by_the_fill_only(model):
    g = torch.Generator().manual_seed(25)
    u8 = torch.randint(0, 256, (2, 48, 80, 3), generator=g, dtype=torch.uint8).to(DEV)
    ing = FrameIngest(size=(64, 64), mode="letterbox", norm="imagenet", channel_order="bgr")
    assert ing.geometry(48, 80) == (13, 0, 38, 64)
    got = model.forward_all_u8(u8, ing, face_stride=STRIDE)
    buf = model.engine._batch_buf("stem_buf", 2, (70, 72, 4))
    x = buf[:, 3:67, 3:67, :3].permute(0, 3, 1, 2).contiguous()          # what the ingest kernel wrote
    fill = torch.tensor(ing.fill) * torch.tensor(ing.a) + torch.tensor(ing.b)
    assert torch.equal(x[:, :, :13].cpu(), fill.view(1, 3, 1, 1).expand(2, 3, 13, 64))
    assert float(x[:, :, 13:51].std()) > 0.5                  # the region holds the image
    want = model.forward_all(x, face_stride=STRIDE)
    for k in want:
        assert _same(got[k], want[k]), k


# ---------------------------------------------------------------------------------- 6. top-down
def _hand_dets():
    dets = torch.zeros(2, 4, 6)
    dets[0, 0, :5] = torch.tensor([10.0, 5.0, 60.0, 90.0, 0.9])
    dets[0, 1, :5] = torch.tensor([70.0, 20.0, 140.0, 100.0, 0.8])       # leaves the frame
    dets[1, 0, :5] = torch.tensor([30.5, 10.25, 90.0, 80.0, 0.7])
    return dets.to(DEV), torch.tensor([2, 1], device=DEV, dtype=torch.int32)


def test_from_detections_u8_equals_from_detections_on_the_float_frames(model):
    g = torch.Generator().manual_seed(26)
    u8 = torch.randint(0, 256, (2, 96, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    x = u8.permute(0, 3, 1, 2).float()
    dets, counts = _hand_dets()
    ing = FrameIngest(norm=I.RAW)
    kw = dict(max_per_frame=2, max_crops=4)
    kp = None
    for compact in (False, True):
        want = TopDownPose(model, compact=compact, box_scale=1.0, **kw).from_detections(x, dets, counts)
        got = TopDownPose(model, compact=compact, **kw).from_detections_u8(u8, dets, counts, ing)
        assert int(got["n_crops"]) == 3 and int(got["status"]) == 0
        assert _same(got["crop_meta"], want["crop_meta"]) and _same(got["keypoints"], want["keypoints"])
        assert kp is None or _same(got["keypoints"], kp)
        kp = got["keypoints"].clone()
    assert float(kp[:3].abs().max()) > 0.0 and float(kp[3:].abs().max()) == 0.0


def test_from_frames_u8_runs_without_a_host_read(model, monkeypatch):
    g = torch.Generator().manual_seed(27)
    u8 = torch.randint(0, 256, (2, 360, 480, 3), generator=g, dtype=torch.uint8).to(DEV)
    ing = FrameIngest(size=(640, 640), mode="letterbox", norm="unit", channel_order="bgr")
    reads = []
    for name in ("cpu", "item", "tolist"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    stride = model.yolo_person.yolo.head.stride
    model.yolo_person.yolo.head.stride = torch.tensor(STRIDE)
    try:
        out = TopDownPose(model, score_thr=0.0, compact=False).from_frames_u8(u8, ing)
    finally:
        model.yolo_person.yolo.head.stride = stride
    assert reads == [] and all(isinstance(v, torch.Tensor) and v.is_cuda for v in out.values())
    people = TopDownPose.results(out)
    assert reads == ["cpu"]                                    # results() is the only read
    monkeypatch.undo()
    assert out["dets"].shape == (2, 300, 6) and out["keypoints"].shape == (16, 17, 3)
    n = int(out["n_crops"])
    counts = out["counts"].cpu()
    assert bool((counts >= 0).all()) and n == min(int(counts.clamp(max=8).sum()), 16)
    assert sum(len(p) for p in people) == n
    meta, kp = out["crop_meta"].cpu()[:n], out["keypoints"].cpu()[:n]
    assert bool(torch.isfinite(kp).all())
    # soft-argmax coordinates lie in [0, 1] of the crop and x = x0 + c * w in fp32: the product's and
    # the sum's roundings are half an ulp of values up to |x0| + w each, and c's own last bit moves
    # the product by 2^-23 w at most: (2^-24 + 2^-24 + 2^-23) (|x0| + w) together
    for c in (0, 1):
        lo, size = meta[:, 2 + c:3 + c], meta[:, 4 + c:5 + c]
        tol = (lo.abs() + size) * 2.0 ** -22
        assert bool(((kp[..., c] >= lo - tol) & (kp[..., c] <= lo + size + tol)).all())
    assert float(meta[:, 4:6].min()) > 0.0 and n > 0
