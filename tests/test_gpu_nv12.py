"""GPU: NV12 frames in (csrc/nv12.hip). Every comparison is an equality of bits.

* ``prpe_nv12_to_rgb`` against ``nv12_to_rgb_ref`` (tests/test_nv12_host.py pins it to a plain
  statement): every (Y, U, V) triple once per table; then the layouts -- 1 x 1 to 33 x 130, a pitch
  wider than the row, two allocations and one surface, BGR, padded output in a sentinel, three frames
  with a frame stride, aligned (8-byte paths) and misaligned (byte paths) planes, and the bytes
  between w and the pitch and below h shown not to be read.
* The four fused kernels against their ``_u8`` twins run on ``to_rgb()``: the ingest over sizes,
  regions, norms and BGR, and against ``ingest_ref`` on ``nv12_sample_ref``; the crop stages over
  the twins' own edge lists (tests/test_gpu_framestages.py, tests/test_gpu_faces.py,
  tests/test_gpu_facealign.py).
* The entry points of the package on an ``NV12Frames`` against the same call on ``to_rgb()``.
"""
import numpy as np
import pytest
import torch

import test_gpu_facealign as GA
import test_gpu_faces as GF
import test_ingest_host as I
import test_nv12_host as NH
from prpe import (CombinedModel, FaceGallery, FrameIngest, NV12Frames, PersonRecognition, PersonTracker, TopDownPose,
                  ops)
from prpe import nv12 as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLES = sorted(N.COEF)
NAN, INF = float("nan"), float("inf")
BT709 = dict(matrix="bt709", range="limited")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _frames(B, H, W, seed, pad=(3, 6), **kw):
    """Random planes on the device inside wider allocations (pitch = row + pad), with their host copies."""
    y, uv = NH.planes(B, H, W, seed)
    hc, wc = uv.shape[1:3]
    g = torch.Generator().manual_seed(seed + 1000)
    ybig = torch.randint(0, 256, (B, H + 2, W + pad[0]), generator=g, dtype=torch.uint8)
    cbig = torch.randint(0, 256, (B, hc + 1, 2 * wc + pad[1]), generator=g, dtype=torch.uint8)
    ybig[:, :H, :W] = y
    cbig[:, :hc, :2 * wc] = uv.reshape(B, hc, 2 * wc)
    yd, cd = ybig.to(DEV), cbig.to(DEV)
    f = NV12Frames(yd[:, :H, :W], cd[:, :hc, :2 * wc].unflatten(2, (wc, 2)), **kw)
    return f, (y, uv)


# ---------------------------------------------------------------------------------- the conversion
@pytest.mark.parametrize("key", TABLES, ids=lambda k: "-".join(k))
def test_conversion_of_every_triple(key):
    """One 4096 x 4096 frame: 2048 x 2048 chroma blocks, each (U, V) pair on 64 of them, whose four
    luma values run through 0..255 -- every (Y, U, V) triple exactly once."""
    blk = torch.arange(2048 * 2048, dtype=torch.int64).view(2048, 2048)
    pair, rep = blk % 65536, blk // 65536                      # rep in 0..63: luma 4 rep .. 4 rep + 3
    uv = torch.stack([pair % 256, pair // 256], dim=-1).to(torch.uint8)[None]
    y = torch.empty(1, 4096, 4096, dtype=torch.uint8)
    for di in (0, 1):
        for dj in (0, 1):
            y[0, di::2, dj::2] = (4 * rep + 2 * di + dj).to(torch.uint8)
    f = NV12Frames(y.to(DEV), uv.to(DEV), matrix=key[0], range=key[1])
    got = f.to_rgb().cpu().numpy()
    want = NH.nv12_to_rgb_ref(y.numpy(), uv.numpy(), N.COEF[key])
    assert got.shape == (1, 4096, 4096, 3) and np.array_equal(got, want)
    triples = (y[0, 0::2, 0::2].to(torch.int64) << 16 | pair).flatten()
    assert int(torch.unique(triples).numel()) == 2048 * 2048    # a quarter here, the other three alike by dj, di
    assert want.min() == 0 and want.max() == 255


SIZES = [(1, 1), (2, 2), (5, 7), (16, 18), (33, 130)]


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("aligned", [False, True], ids=["bytes", "wide"])
def test_conversion_layouts(hw, aligned):
    H, W = hw
    B = 3
    hc, wc = (H + 1) // 2, (W + 1) // 2
    coef = N.COEF[("bt601", "limited")]
    kw = dict(matrix="bt601", range="limited")
    # one decoder surface per frame: luma rows, a gap row, chroma rows, at one pitch; the bytes past w
    # and the rows below h hold random values
    pitch = ((W + 15) // 8) * 8 if aligned else 2 * wc + 6
    pitch += 2 if not aligned and pitch % 8 == 0 else 0
    uv_row = H + 1 if not aligned else ((H + 7) // 8) * 8
    rows = uv_row + hc + 1
    g = torch.Generator().manual_seed(H * 131 + W)
    surf = torch.randint(0, 256, (B, rows, pitch), generator=g, dtype=torch.uint8)
    if aligned and (rows * pitch) % 8:
        pytest.fail("the aligned surface must have an 8-byte frame stride")
    y, uv = surf[:, :H, :W].clone(), surf[:, uv_row:uv_row + hc, :2 * wc].reshape(B, hc, wc, 2).clone()
    want = torch.from_numpy(NH.nv12_to_rgb_ref(y.numpy(), uv.numpy(), coef))
    sd = surf.to(DEV)
    f = NV12Frames.from_surface(sd, H, W, uv_row=uv_row, **kw)
    assert f.y.data_ptr() == sd.data_ptr() and (f.y.data_ptr() % 8 == 0 and pitch % 8 == 0) == aligned
    got = f.to_rgb()
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    assert torch.equal(f.to_rgb("bgr").cpu(), want.flip(3))
    # the same planes with everything else zeroed: the padding and the rows below h are not read
    clean = torch.zeros_like(surf)
    clean[:, :H, :W] = y
    clean[:, uv_row:uv_row + hc, :2 * wc] = uv.reshape(B, hc, 2 * wc)
    assert torch.equal(NV12Frames.from_surface(clean.to(DEV), H, W, uv_row=uv_row, **kw).to_rgb().cpu(), want)
    # two allocations, each with its own pitch
    f2, (y2, uv2) = _frames(B, H, W, seed=H + W, pad=(8 - W % 8 if aligned else 3, 6), **kw)
    want2 = torch.from_numpy(NH.nv12_to_rgb_ref(y2.numpy(), uv2.numpy(), coef))
    assert torch.equal(f2.to_rgb().cpu(), want2)
    # a padded output inside a sentinel: row padding, a frame stride, an extra frame; nothing else written
    opad = 8 - (3 * W) % 8 if aligned else 5
    outer = torch.full((B + 1, H + 1, 3 * W + opad), 0xA5, dtype=torch.uint8, device=DEV)
    out = outer[:B, :H, :3 * W].unflatten(2, (W, 3))
    assert f.to_rgb(out=out) is out
    host = outer.cpu()
    assert torch.equal(host[:B, :H, :3 * W].reshape(B, H, W, 3), want)
    mask = torch.ones_like(host, dtype=torch.bool)
    mask[:B, :H, :3 * W] = False
    assert bool((host[mask] == 0xA5).all())
    # one frame of the batch alone
    one = NV12Frames(f.y[1:2], f.uv[1:2], **kw)
    assert torch.equal(one.to_rgb().cpu(), want[1:2])


# ---------------------------------------------------------------------------------- the ingest
RAW = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
INGEST_CASES = {
    "equal_size": ((12, 18), dict(size=(12, 18), mode="stretch", norm=RAW)),
    "up_1.5": ((12, 18), dict(size=(18, 27), mode="stretch")),
    "down_2": ((24, 36), dict(size=(12, 18), mode="stretch")),
    "down_2.7": ((27, 54), dict(size=(10, 20), mode="stretch")),
    "odd_source": ((13, 17), dict(size=(20, 30), mode="stretch", norm="half")),
    "odd_source_equal": ((13, 17), dict(size=(13, 17), mode="stretch", norm=RAW)),
    "1x1": ((1, 1), dict(size=(8, 8), mode="stretch")),
    "letterbox_fill": ((10, 30), dict(size=(32, 48), mode="letterbox", fill=(7, 114, 250))),
    "letterbox_tall": ((31, 9), dict(size=(24, 40), mode="letterbox", fill=33)),
    "stretch": ((9, 23), dict(size=(16, 300), mode="stretch")),
    "imagenet": ((14, 22), dict(size=(16, 24), mode="letterbox", norm="imagenet")),
    "bgr": ((14, 22), dict(size=(16, 24), mode="letterbox", norm="imagenet", channel_order="bgr", fill=(1, 2, 3))),
}


def _ingest(op, frames, ing, Hs, Ws, B, **kw):
    H, W = ing.size
    outer = torch.full((B, H + 6, W + 8, 4), -7.0, device=DEV)
    amax = torch.zeros(B, device=DEV)
    op(frames, outer[:, 3:3 + H, 3:3 + W, :], ing.geometry(Hs, Ws), ing.a, ing.b, ing.fill, y_amax=amax, **kw)
    return outer.cpu(), amax.cpu()


@pytest.mark.parametrize("name", list(INGEST_CASES))
def test_frame_ingest_nv12_has_the_u8_route_bits(name):
    (Hs, Ws), kw = INGEST_CASES[name]
    ing = FrameIngest(**kw)
    B = 3
    f, pl = _frames(B, Hs, Ws, seed=len(name) * 7 + Hs, **BT709)
    H, W = ing.size
    rgb = f.to_rgb(ing.channel_order)
    want, want_amax = _ingest(ops.frame_ingest, rgb, ing, Hs, Ws, B, swap_rb=ing.swap_rb)
    got, amax = _ingest(ops.frame_ingest_nv12, f, ing, Hs, Ws, B)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(amax), _bits(want_amax))
    inner = got[:, 3:3 + H, 3:3 + W, :]
    border = torch.ones_like(got, dtype=torch.bool)
    border[:, 3:3 + H, 3:3 + W, :] = False
    assert bool((got[border] == -7.0).all()) and float(inner[..., 3].abs().max()) == 0.0
    assert torch.equal(_bits(amax), _bits(inner.abs().amax(dim=(1, 2, 3))))
    # the host restatement on the converted frames, in raw units: the bound of tests/test_gpu_ingest.py,
    # 2^-14 (one ulp of [128, 256) per lerp stage and per rounded weight; coordinates are fp64)
    conv = NH.nv12_sample_ref(pl, f.coef)
    raw = FrameIngest(**dict(kw, norm=RAW, channel_order="rgb"))
    got_raw, _ = _ingest(ops.frame_ingest_nv12, f, raw, Hs, Ws, B)
    err = float((got_raw[:, 3:3 + H, 3:3 + W, :3].double() - I.ingest_ref(conv, raw)).abs().max())
    print(f"frame_ingest_nv12 {name}: max|d| to ingest_ref {err:.3e}, bound {2.0 ** -14:.3e}")
    assert err <= 2.0 ** -14
    if name in ("equal_size", "odd_source_equal"):
        assert torch.equal(inner[..., :3], conv.float())          # the bits of rgb.float() * 1 + 0
    # batch positions are independent, and two runs agree
    one = NV12Frames(f.y[2:3], f.uv[2:3], **BT709)
    solo, solo_amax = _ingest(ops.frame_ingest_nv12, one, ing, Hs, Ws, 1)
    assert torch.equal(_bits(solo[0]), _bits(got[2])) and torch.equal(_bits(solo_amax), _bits(amax[2:3]))
    again, again_amax = _ingest(ops.frame_ingest_nv12, f, ing, Hs, Ws, B)
    assert torch.equal(_bits(again), _bits(got)) and torch.equal(_bits(again_amax), _bits(amax))


# ---------------------------------------------------------------------------------- the crop stages
H1, W1 = 40, 56
CROP_WINS = [                                                      # tests/test_gpu_framestages.py's lists
    (1, (-1.0, -1.0, 192.0, 256.0)), (0, (-500.0, 5.0, 100.0, 20.0)), (-1, (0.0, 0.0, 0.0, 0.0)),
    (0, (5.0, 500.0, 20.0, 100.0)), (2, (20.25, 4.0, 0.0, 30.0)), (7, (12.0, 3.0, 20.0, 26.0)),
    (2, (-1.5, -1.5, 60.0, 44.0)), (0, (5.0, -500.0, 20.0, 100.0)), (0, (500.0, 5.0, 100.0, 20.0)),
    (0, (10.0, 5.0, 30.0, 28.0)), (1, (NAN, 5.0, 30.0, 28.0)), (1, (10.0, NAN, 30.0, 28.0)), (1, (10.0, 5.0, NAN, 28.0)),
    (1, (10.0, 5.0, 30.0, NAN)), (1, (INF, 5.0, 30.0, 28.0)), (1, (-INF, 5.0, 30.0, 28.0)), (1, (10.0, INF, 30.0, 28.0)),
    (1, (10.0, 5.0, INF, 28.0)), (1, (10.0, 5.0, 30.0, -INF)), (1, (-INF, 5.0, INF, 28.0)), (1, (NAN, NAN, NAN, NAN)),
    (0, (0.0, 0.0, float(W1), float(H1))), (1, (-45.0, -35.0, 150.0, 112.5)), (2, (29.5, 19.5, 1.0, 1.0)),
    (1, (float(W1 - 1), float(H1 - 1), 192.0, 256.0)), (1, (float(W1), float(H1), 192.0, 256.0))]


def _crop_both(f, rgb, wins, n_crops, ing, swap=False):
    S = len(wins) + 1
    meta = GF._meta(wins, S).to(DEV)
    n = torch.tensor([n_crops], device=DEV, dtype=torch.int32)
    bufs = []
    for _ in range(2):
        b = torch.zeros(S, 260, 196, 4, device=DEV)
        b[:, 2:-2, 2:-2, :3] = 1.0                            # stale crops everywhere
        bufs.append(b)
    ops.crop_resize_u8(rgb, meta, n, bufs[0], ing.a, ing.b, swap)
    ops.crop_resize_nv12(f, meta, n, bufs[1], ing.a, ing.b)
    return bufs[0].cpu(), bufs[1].cpu()


@pytest.mark.parametrize("hw,n_crops", [((H1, W1), None), ((39, 55), None), ((H1, W1), 100), ((H1, W1), 3), ((H1, W1), 0),
                                        ((H1, W1), -3), ((1, 1), None), ((1, 9), None), ((7, 1), None)],
                         ids=["40x56", "39x55_odd", "n_above_max", "n_3", "n_0", "n_negative", "1x1", "1x9", "7x1"])
def test_crop_resize_nv12_has_the_u8_route_bits(hw, n_crops):
    H, W = hw
    f, _ = _frames(3, H, W, seed=71 + H, **BT709)
    ing = FrameIngest(norm="imagenet")
    wins = CROP_WINS if min(hw) > 1 else [(0, (0.0, 0.0, float(W), float(H))), (1, (-2.0, -1.5, 12.0, 4.0)),
                                          (1, (-1.5, -2.0, 4.0, 12.0)), (2, (0.25, 0.25, 0.75, 1.0)), (3, (0.0, 0.0, 1.0, 1.0))]
    want, got = _crop_both(f, f.to_rgb(), wins, len(wins) if n_crops is None else n_crops, ing)
    assert torch.equal(_bits(got), _bits(want))
    if n_crops is None:
        assert float(want[0].abs().max()) > 1.0 and float(want[len(wins)].abs().max()) == 0.0
    want, got = _crop_both(f, f.to_rgb("bgr"), wins, len(wins) if n_crops is None else n_crops, ing, swap=True)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("out_hw", [(112, 112), (9, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("hw", [(40, 56), (39, 55)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_roi_resize_and_warp_nv12_have_the_u8_route_bits(out_hw, hw):
    oh, ow = out_hw
    H, W = hw
    f, _ = _frames(3, H, W, seed=5 + H, **BT709)
    rgb = f.to_rgb()
    ing = FrameIngest(norm="imagenet")
    good, zero = GF._windows(out_hw)
    edge = [(1, (-1.0, -1.0, float(ow), float(oh))), (1, (float(W - 1), float(H - 1), float(ow), float(oh))),
            (1, (float(W), float(H), float(ow), float(oh))), (0, (20.25, 4.0, 0.0, 30.0)), (2, (29.5, 19.5, 1.0, 1.0))]

    def run(fn, frames, meta, n, *args, **kw):
        S = meta.shape[0]
        outer = torch.full((S + 1, oh + 3, ow + 5, 4), 7.0, device=DEV)
        amax = torch.zeros(S, device=DEV)
        amax[1] = 1e6                                       # a slot that already holds more keeps it
        fn(frames, meta, n, *args, outer[:S, 1:1 + oh, 2:2 + ow, :], a=ing.a, b=ing.b, y_amax=amax, **kw)
        return outer.cpu(), amax.cpu()

    rows = good + zero + edge
    for n_crops in (len(rows), len(rows) + 50, 4):
        meta = GF._meta(rows, len(rows) + 2)
        meta.view(torch.int32)[len(rows), 0] = 0             # a stale, valid-looking row past n_crops
        meta[len(rows), 2:6] = torch.tensor([5.0, 5.0, 20.0, 20.0])
        meta, n = meta.to(DEV), torch.tensor([n_crops], device=DEV, dtype=torch.int32)
        want, want_amax = run(ops.roi_resize_u8, rgb, meta, n)
        got, amax = run(ops.roi_resize_nv12, f, meta, n)
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(amax), _bits(want_amax))
        assert float(amax[1]) == 1e6 and float(amax[0]) > 0.5
    # the warp: flagged rows (rotations, partly and wholly outside, wild coefficients), unflagged rows
    # and empty slots in one launch
    wrows, n_held = GA._warps(out_hw)
    S = len(wrows) + 1
    meta = GF._meta([(fr, w) for fr, _, w in wrows] + [(0, wrows[0][2])], S).to(DEV)
    warp = GA._warp_rows(S, [(s, c) for s, (_, c, _) in enumerate(wrows) if c is not None] + [(S - 1, wrows[0][1])]).to(DEV)
    n = torch.tensor([len(wrows)], device=DEV, dtype=torch.int32)
    want, want_amax = run(ops.roi_warp_u8, rgb, meta, n, warp)
    got, amax = run(ops.roi_warp_nv12, f, meta, n, warp)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(amax), _bits(want_amax))
    assert float(amax[:n_held].min()) > 0.5 and not bool(torch.isnan(got).any())
    plain, _ = run(ops.roi_resize_nv12, f, meta, n)
    assert not torch.equal(_bits(plain[1]), _bits(got[1]))   # the rotated slot is not its window's resize
    bgr, bgr_amax = run(ops.roi_warp_u8, f.to_rgb("bgr"), meta, n, warp, swap_rb=True)
    assert torch.equal(_bits(got), _bits(bgr)) and torch.equal(_bits(amax), _bits(bgr_amax))


# ---------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model(state_dict):
    m = CombinedModel(state_dict, device=DEV)
    saved = GF._strides(m, ("yolo_face", "yolo_person"))
    yield m
    for b, s in saved.items():
        getattr(m, b).yolo.head.stride = s


@pytest.fixture(scope="module")
def video():
    """Two batches of [2, 90, 122] NV12 frames on one decoder-like surface each."""
    out = []
    for seed in (61, 62):
        g = torch.Generator().manual_seed(seed)
        surf = torch.randint(0, 256, (2, 96 + 45, 128), generator=g, dtype=torch.uint8).to(DEV)
        out.append(NV12Frames.from_surface(surf, 90, 122, uv_row=96))
    return out


def _flat(out, prefix=""):
    if isinstance(out, dict):
        r = {}
        for k, v in out.items():
            r.update(_flat(v, f"{prefix}{k}."))
        return r
    if isinstance(out, (list, tuple)):
        r = {}
        for k, v in enumerate(out):
            r.update(_flat(v, f"{prefix}{k}."))
        return r
    if hasattr(out, "heatmaps"):
        return {prefix + "heatmaps": out.heatmaps}
    return {prefix[:-1]: out} if isinstance(out, torch.Tensor) else {}


def _equal_outputs(got, want):
    a, b = _flat(got), _flat(want)
    assert set(a) == set(b) and a
    bad = [k for k in a if not _same(a[k].cpu(), b[k].cpu())]
    assert not bad, bad


ING = dict(size=(64, 96), mode="letterbox", norm="unit")


def test_forward_all_u8_on_nv12(model, video):
    nv = video[0]
    ing = FrameIngest(**ING)
    want = model.forward_all_u8(nv.to_rgb(), ing, face_stride=GF.STRIDE)
    got = model.forward_all_u8(nv, ing, face_stride=GF.STRIDE)
    _equal_outputs(got, want)
    bgr = FrameIngest(**dict(ING, channel_order="bgr"))
    _equal_outputs(model.forward_all_u8(nv, bgr, face_stride=GF.STRIDE),
                   model.forward_all_u8(nv.to_rgb("bgr"), bgr, face_stride=GF.STRIDE))
    _equal_outputs(model.forward_all_u8(nv, bgr, face_stride=GF.STRIDE), want)       # NV12 output is RGB either way


def test_forward_u8_antialias_on_nv12(model, video):
    nv = video[1]
    aa = FrameIngest(**dict(ING, size=(32, 48), antialias=True))
    for ing in (aa, FrameIngest(**dict(ING, size=(32, 48), antialias=True, channel_order="bgr"))):
        want = model.forward_u8(nv.to_rgb(ing.channel_order), ing)
        got = model.forward_u8(nv, ing)
        _equal_outputs(got, want)
    keys = [k for k in model.engine._aux if isinstance(k, tuple) and k[0] == "nv12_rgb"]
    assert keys == [("nv12_rgb", 2, 90, 122)]
    one = NV12Frames(nv.y[:1], nv.uv[:1])
    model.forward_u8(one, aa)                                # another batch size replaces the staging buffer
    keys = [k for k in model.engine._aux if isinstance(k, tuple) and k[0] == "nv12_rgb"]
    assert keys == [("nv12_rgb", 1, 90, 122)]
    plain = model.forward_u8(nv, FrameIngest(**dict(ING, size=(32, 48))))
    assert not _same(_flat(plain)[next(iter(_flat(plain)))].cpu(), _flat(got)[next(iter(_flat(got)))].cpu())


def test_top_down_pose_on_nv12(model, video):
    nv = video[0]
    ing = FrameIngest(**ING)
    pose = TopDownPose(model, score_thr=0.0, max_per_frame=2)
    want = pose.from_frames_u8(nv.to_rgb(), ing)
    got = pose.from_frames_u8(nv, ing)
    _equal_outputs(got, want)
    assert int(got["n_crops"]) > 0 and bool(torch.isfinite(got["keypoints"]).all())


@pytest.mark.parametrize("align", [False, True], ids=["plain", "align"])
def test_person_recognition_and_tracker_on_nv12(model, video, align):
    ing = FrameIngest(**ING)

    def build():
        gallery = FaceGallery(dim=512, capacity=4, device=DEV)
        gallery.add(torch.randn(2, 512, generator=torch.Generator().manual_seed(44)).to(DEV), [5, 6])
        return PersonRecognition(model, gallery, pose=dict(score_thr=0.0, max_per_frame=2), kp_thr=0.0,
                                 faces=dict(score_thr=0.0, min_size=1.0, max_per_frame=2, threshold=-1.0), align=align)
    pr = build()
    want = pr.from_frames_u8(video[0].to_rgb(), ing)
    got = pr.from_frames_u8(video[0], ing)
    _equal_outputs(got, want)
    assert int(got["pose"]["n_crops"]) > 0 and int(got["faces"]["n_crops"]) > 0
    ta, tb = PersonTracker(build(), new_thr=0.0), PersonTracker(build(), new_thr=0.0)
    for nv in video:                                         # two consecutive batches: the state carries over
        _equal_outputs(ta.from_frames_u8(nv, ing), tb.from_frames_u8(nv.to_rgb(), ing))
