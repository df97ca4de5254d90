"""CPU: the uint8 ingest stage (prpe.ingest, csrc/ingest.hip) as far as the host goes -- the
letterbox geometry, the coordinate maps, a plain-torch restatement of the kernel's semantics
(``ingest_ref``, the yardstick tests/test_gpu_ingest.py holds the kernel to), the ABI table, the
library's refusals before launch and the argument checks of the ops wrappers."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

from prpe import FrameIngest, _lib


def ingest_ref(u8, ingest, dtype=torch.float64, region=None):
    """prpe_frame_ingest in plain torch on the host: u8 [B, Hs, Ws, 3] (source channel order) ->
    [B, H, W, 3] of ``dtype``: F.interpolate(bilinear, align_corners=False, antialias=False) of the
    raw values into the region (``ingest.geometry``'s, or the given (top, left, nh, nw)), the fill
    outside it, then raw * a + b."""
    B, Hs, Ws, _ = u8.shape
    H, W = ingest.size
    top, left, nh, nw = ingest.geometry(Hs, Ws) if region is None else region
    x = u8.cpu().permute(0, 3, 1, 2).to(dtype)
    if ingest.swap_rb:
        x = x.flip(1)
    canvas = torch.tensor(ingest.fill, dtype=dtype).view(1, 3, 1, 1).repeat(B, 1, H, W)
    canvas[:, :, top:top + nh, left:left + nw] = F.interpolate(x, size=(nh, nw), mode="bilinear",
                                                               align_corners=False, antialias=False)
    a = torch.tensor(ingest.a, dtype=dtype).view(1, 3, 1, 1)
    b = torch.tensor(ingest.b, dtype=dtype).view(1, 3, 1, 1)
    return (canvas * a + b).permute(0, 2, 3, 1).contiguous()


RAW = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))          # norm = (a, b): the raw 0..255 values


# ---------------------------------------------------------------------------------- geometry
def test_geometry_letterbox_and_stretch():
    lb = FrameIngest(size=(640, 640), mode="letterbox")
    assert lb.geometry(1080, 1920) == (140, 0, 360, 640)
    assert lb.geometry(720, 1280) == (140, 0, 360, 640)
    assert lb.geometry(1920, 1080) == (0, 140, 640, 360)            # portrait
    assert lb.geometry(500, 500) == (0, 0, 640, 640)                # square: the whole frame
    assert lb.geometry(100, 50) == (0, 160, 640, 320)               # smaller than the target: magnified
    assert lb.geometry(1, 5000) == (319, 0, 1, 640)                 # a sliver keeps one row
    assert FrameIngest(size=(32, 48)).geometry(37, 53) == (0, 1, 32, 46)
    assert FrameIngest(size=(48, 32)).geometry(37, 53) == (13, 0, 22, 32)
    st = FrameIngest(size=(384, 640), mode="stretch")
    assert st.geometry(1080, 1920) == (0, 0, 384, 640) and st.geometry(7, 9) == (0, 0, 384, 640)
    for Hs, Ws in ((1080, 1920), (333, 77), (5, 4000), (640, 640), (641, 639)):
        top, left, nh, nw = lb.geometry(Hs, Ws)
        assert 1 <= nh <= 640 and 1 <= nw <= 640 and top == (640 - nh) // 2 and left == (640 - nw) // 2
        assert max(nh, nw) == 640                                   # the longer side fills the frame
    with pytest.raises(ValueError):
        lb.geometry(0, 10)
    for bad in (dict(mode="crop"), dict(channel_order="gbr"), dict(norm="minmax"), dict(size=(0, 4)),
                dict(norm=((1, 1), (0, 0))), dict(fill=(1, 2))):
        with pytest.raises(ValueError):
            FrameIngest(**bad)


def test_norm_presets_fold_mean_and_std_in_fp32():
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).float())
    u = FrameIngest(norm="unit")
    assert u.a == (f32(1 / 255),) * 3 and u.b == (0.0, 0.0, 0.0) and u.fill == (114.0,) * 3 and not u.swap_rb
    im = FrameIngest(norm="imagenet", channel_order="bgr", fill=(0, 1, 2))
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    assert im.a == tuple(f32(1 / (255 * s)) for s in std) and im.b == tuple(f32(-m / s) for m, s in zip(mean, std))
    assert im.swap_rb and im.fill == (0.0, 1.0, 2.0)
    h = FrameIngest(norm="half")
    assert h.a == (f32(1 / 127.5),) * 3 and h.b == (-1.0,) * 3
    # raw 255 -> (1 - mean) / std, raw 0 -> -mean / std, to fp32 rounding
    assert abs(255 * im.a[0] + im.b[0] - (1 - 0.485) / 0.229) < 1e-6
    c = FrameIngest(norm=((2, 3, 4), (0.1, 0.2, 0.3)))
    assert c.a == (2.0, 3.0, 4.0) and c.b == (f32(0.1), f32(0.2), f32(0.3))


def test_to_source_and_to_model_are_inverse():
    g = torch.Generator().manual_seed(11)
    for ing, (Hs, Ws) in ((FrameIngest((640, 640)), (1080, 1920)), (FrameIngest((640, 640)), (1920, 1080)),
                          (FrameIngest((384, 640), mode="stretch"), (720, 1280)), (FrameIngest((64, 64)), (10, 14))):
        top, left, nh, nw = ing.geometry(Hs, Ws)
        p = torch.rand(5, 7, 4, generator=g) * torch.tensor([Ws, Hs, Ws, Hs], dtype=torch.float32)
        back = ing.to_source(ing.to_model(p, Hs, Ws), Hs, Ws)
        assert back.dtype == torch.float32 and back.shape == p.shape
        # two fp32 operations each way on values up to max(Hs, Ws): a few ulp of that
        assert float((back - p).abs().max()) <= 8 * max(Hs, Ws) * 2.0 ** -24
        pts = p[..., :2]
        assert torch.equal(ing.to_model(pts, Hs, Ws), ing.to_model(p, Hs, Ws)[..., :2])
        # the region's corners are the source's corners
        corners = torch.tensor([[left, top, left + nw, top + nh]], dtype=torch.float32)
        want = torch.tensor([[0.0, 0.0, Ws, Hs]])
        assert float((ing.to_source(corners, Hs, Ws) - want).abs().max()) <= 1e-3
    with pytest.raises(ValueError):
        FrameIngest().to_source(torch.zeros(3, 3), 10, 10)


# ---------------------------------------------------------------------------------- the restatement
def test_ingest_ref_on_a_hand_computed_case():
    """2 x 2 -> 4 x 4: sample positions -0.25 (clamped to 0), 0.25, 0.75, 1.25 (clamped to 1) on both
    axes, so the weights are 0, 1/4, 3/4, 1; horizontal lerp first, then vertical."""
    u8 = torch.tensor([[[[0, 10, 20], [100, 10, 60]], [[200, 10, 100], [40, 10, 20]]]], dtype=torch.uint8)
    y = ingest_ref(u8, FrameIngest(size=(4, 4), mode="stretch", norm=RAW))
    assert y.shape == (1, 4, 4, 3) and y.dtype == torch.float64
    want0 = torch.tensor([[0.0, 25.0, 75.0, 100.0], [50.0, 58.75, 76.25, 85.0], [150.0, 126.25, 78.75, 55.0],
                          [200.0, 160.0, 80.0, 40.0]], dtype=torch.float64)
    assert torch.equal(y[0, :, :, 0], want0)
    assert torch.equal(y[0, :, :, 1], torch.full((4, 4), 10.0, dtype=torch.float64))     # constant stays constant
    # bgr: output channel c reads source channel 2 - c; a, b belong to the output channel
    z = ingest_ref(u8, FrameIngest(size=(4, 4), mode="stretch", norm=((1, 1, 2), (0, 0, 1)), channel_order="bgr"))
    assert torch.equal(z[0, :, :, 2], want0 * 2 + 1) and torch.equal(z[0, :, :, 0], y[0, :, :, 2])


def test_ingest_ref_letterbox_fill_and_identity():
    g = torch.Generator().manual_seed(12)
    u8 = torch.randint(0, 256, (2, 4, 8, 3), generator=g, dtype=torch.uint8)
    ing = FrameIngest(size=(8, 8), mode="letterbox", norm="imagenet", fill=(114, 0, 255))
    assert ing.geometry(4, 8) == (2, 0, 4, 8)                       # same size: the region is a copy
    y = ingest_ref(u8, ing, torch.float32)
    a, b = torch.tensor(ing.a), torch.tensor(ing.b)
    assert torch.equal(y[:, 2:6], u8.float() * a + b)
    fill = torch.tensor(ing.fill) * a + b
    assert torch.equal(y[:, :2], fill.expand(2, 2, 8, 3)) and torch.equal(y[:, 6:], fill.expand(2, 2, 8, 3))


# ---------------------------------------------------------------------------------- the edges
# name -> ((Hs, Ws) of the source, (H, W) of the model frame, region (top, left, nh, nw)): the
# frame_ingest shapes tests/test_gpu_framestages.py sends to the kernel
INGEST_EDGES = {
    "source_1x1": ((1, 1), (5, 7), (0, 0, 5, 7)),               # xb == xa and yb == ya everywhere
    "source_one_row": ((1, 9), (6, 11), (0, 0, 6, 11)),         # Hs == 1
    "source_one_column": ((9, 1), (11, 6), (0, 0, 11, 6)),      # Ws == 1
    "region_one_row": ((5, 40), (8, 16), (3, 0, 1, 16)),        # nh == 1: the source's middle row
    "region_one_column": ((40, 5), (8, 16), (0, 5, 8, 1)),      # nw == 1
    "strong_downscale": ((97, 131), (3, 5), (0, 0, 3, 5)),
    "odd_region_off_every_edge": ((10, 14), (16, 24), (3, 5, 9, 11)),
    "narrow_with_whole_row_groups": ((10, 14), (16, 40), (0, 0, 16, 40)),   # W < 256, H == 2 * 8
    # region = source size: every weight is 0 and the result is the source pixel
    "identity_1x1": ((1, 1), (1, 1), (0, 0, 1, 1)),
    "identity_whole_row_groups": ((16, 40), (16, 40), (0, 0, 16, 40)),
    "identity_odd_region": ((9, 11), (16, 24), (3, 5, 9, 11)),
}


def edge_source(name):
    Hs, Ws = INGEST_EDGES[name][0]
    g = torch.Generator().manual_seed(31 + sorted(INGEST_EDGES).index(name))
    u8 = torch.randint(0, 256, (2, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    u8[0, 0, 0, 0], u8[1, -1, -1, 2] = 255, 0
    return u8


def ingest_plain(u8, size, region, a, b, fill):
    """The resize rule as a Python loop in float64, written apart from ``ingest_ref``: an output
    pixel centre (i + 0.5) maps to (i + 0.5) * Hs / nh - 0.5 in the source, clamped below at 0;
    the second tap is the next pixel or, on the last one, the same; weights 1 - t and t, the
    horizontal pair first (torch's upsample_bilinear2d with align_corners=False)."""
    import math
    B, Hs, Ws, _ = u8.shape
    H, W = size
    top, left, nh, nw = region
    out = torch.empty(B, H, W, 3, dtype=torch.float64)
    src = u8.double()
    for i in range(H):
        for j in range(W):
            if not (top <= i < top + nh and left <= j < left + nw):
                for c in range(3):
                    out[:, i, j, c] = fill[c] * a[c] + b[c]
                continue
            sy = max((i - top + 0.5) * (Hs / nh) - 0.5, 0.0)
            sx = max((j - left + 0.5) * (Ws / nw) - 0.5, 0.0)
            ya, xa = min(math.floor(sy), Hs - 1), min(math.floor(sx), Ws - 1)
            yb, xb = min(ya + 1, Hs - 1), min(xa + 1, Ws - 1)
            ty, tx = sy - ya, sx - xa
            for c in range(3):
                p, q = src[:, ya, xa, c] * (1 - tx) + src[:, ya, xb, c] * tx, \
                    src[:, yb, xa, c] * (1 - tx) + src[:, yb, xb, c] * tx
                out[:, i, j, c] = (p * (1 - ty) + q * ty) * a[c] + b[c]
    return out


@pytest.mark.parametrize("name", sorted(INGEST_EDGES))
def test_ingest_ref_at_the_edges_equals_the_plain_statement(name):
    """``ingest_ref`` (F.interpolate in float64) against ``ingest_plain`` at the degenerate
    geometries. Both are float64 throughout but order the four products differently, so they
    agree to a few fp64 roundings at 255, not bit for bit: the bound is 2^-40 raw units, 2^-26 of
    the 2^-14 the kernel is held to. Fill pixels are exact."""
    (Hs, Ws), size, region = INGEST_EDGES[name]
    u8 = edge_source(name)
    ing = FrameIngest(size=size, mode="stretch", norm=RAW, fill=(114, 3, 250))
    ref = ingest_ref(u8, ing, region=region)
    plain = ingest_plain(u8, size, region, ing.a, ing.b, ing.fill)
    assert ref.shape == plain.shape == (2, *size, 3)
    assert float((ref - plain).abs().max()) <= 2.0 ** -40
    top, left, nh, nw = region
    inside = torch.zeros(size, dtype=torch.bool)
    inside[top:top + nh, left:left + nw] = True
    assert torch.equal(ref[:, ~inside], plain[:, ~inside])
    if not bool(inside.all()):
        assert torch.equal(ref[0][~inside][0], torch.tensor(ing.fill, dtype=torch.float64))
    assert float(ref[:, inside].max()) > 150.0 and float(ref[:, inside].min()) >= 0.0
    # one source row / column: every output row / column of the region is the same, to the
    # yardstick's own fp64 rounding (its weights 1 - t and t need not sum to 1 exactly)
    if Hs == 1:
        assert float((ref[:, top:top + nh] - ref[:, top:top + 1]).abs().max()) <= 2.0 ** -40
    if Ws == 1:
        assert float((ref[:, :, left:left + nw] - ref[:, :, left:left + 1]).abs().max()) <= 2.0 ** -40
    if (Hs, Ws) == (1, 1):
        assert float((ref - u8.double().expand(2, *size, 3)).abs().max()) <= 2.0 ** -40
    if name == "region_one_row":                      # (0 + 0.5) * 5 / 1 - 0.5 = 2: source row 2, weight 0
        sub = FrameIngest(size=(1, 16), mode="stretch", norm=RAW)
        assert torch.equal(ref[:, 3:4], ingest_ref(u8[:, 2:3], sub))


# ---------------------------------------------------------------------------------- ABI
def test_abi_table_has_the_ingest_entry_points():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert _lib.ABI_VERSION == 12
    assert int(re.search(r"#define PRPE_ABI_VERSION (\d+)", header).group(1)) == 12
    for name, nargs in (("prpe_frame_ingest", 12), ("prpe_crop_resize_u8", 9)):
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/prpe.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.lib(), name)
    assert "typedef struct prpe_view_u8" in header
    assert _lib.lib().prpe_abi_version() == 12


def test_library_rejects_bad_ingest_arguments_before_launch():
    L = _lib.lib()
    p = 0x1000
    f3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    src = _lib.View(p, 2, 8, 10, 3, 240, 30, 3, 1)
    dst = _lib.View(p, 2, 16, 16, 4, 2048, 96, 4, 1)                # the interior of a wider buffer

    def ingest(s=src, d=dst, region=(0, 0, 16, 16), a=f3, b=f3, fill=f3, amax=None):
        return L.prpe_frame_ingest(C.byref(s) if s is not None else None, C.byref(d) if d is not None else None,
                                   *region, a, b, fill, 0, amax, None)

    def with_(v, **kw):
        w = _lib.View(v.ptr, v.n, v.h, v.w, v.c, v.sn, v.sh, v.sw, v.sc)
        for k, val in kw.items():
            setattr(w, k, val)
        return w

    assert ingest(s=None) == -22 and ingest(d=None) == -22          # null pointers
    assert ingest(s=with_(src, ptr=None)) == -22 and ingest(d=with_(dst, ptr=None)) == -22
    assert ingest(a=None) == -22 and ingest(b=None) == -22 and ingest(fill=None) == -22
    assert ingest(s=with_(src, n=3)) == -22                          # mismatched n
    assert ingest(s=with_(src, c=4)) == -22                          # source is not 3 channels
    assert ingest(d=with_(dst, c=3)) == -22                          # destination is not 4 channels
    assert ingest(d=with_(dst, sc=2)) == -22                         # ... not contiguous ones
    assert ingest(d=with_(dst, sw=6)) == -22 and ingest(d=with_(dst, sh=98)) == -22
    assert ingest(d=with_(dst, ptr=p + 4)) == -22                    # not 16-byte aligned
    for region in ((0, 0, 0, 16), (0, 0, 16, 0), (-1, 0, 16, 16), (0, -1, 16, 16), (1, 0, 16, 16), (0, 1, 16, 16),
                   (0, 0, 17, 16), (4, 4, 8, 13), (2 ** 31 - 1, 0, 2, 16)):
        assert ingest(region=region) == -22, region                  # empty, or not inside H x W
    assert ingest(s=with_(src, h=0)) == -22 and ingest(s=with_(src, w=0)) == -22    # a source side below 1
    assert ingest(d=with_(dst, h=0)) == -22 and ingest(d=with_(dst, w=-3)) == -22
    big = 2 ** 30                                                    # n * ceil(h / 8) workgroups: past 31 bits
    assert ingest(s=with_(src, n=big), d=with_(dst, n=big, h=64), region=(0, 0, 64, 16)) == -22

    def crop(s=src, meta=p, n=p, max_crops=4, a=f3, b=f3, crops=p):
        return L.prpe_crop_resize_u8(C.byref(s) if s is not None else None, meta, n, max_crops, a, b, 0, crops, None)

    assert crop(s=None) == -22 and crop(s=with_(src, ptr=None)) == -22 and crop(meta=None) == -22
    assert crop(n=None) == -22 and crop(crops=None) == -22 and crop(a=None) == -22 and crop(b=None) == -22
    assert crop(s=with_(src, c=4)) == -22 and crop(s=with_(src, h=0)) == -22 and crop(s=with_(src, n=0)) == -22
    assert crop(max_crops=0) == -22 and crop(max_crops=2 ** 27) == -22              # no slot; grid past 31 bits
    assert crop(crops=p + 8) == -22                                  # unaligned buffer


# ---------------------------------------------------------------------------------- ops
def test_ops_validate_ingest_arguments_before_any_launch():
    from prpe import ops
    y = torch.zeros(1, 8, 8, 4)
    args = ((0, 0, 8, 8), (1, 1, 1), (0, 0, 0))
    with pytest.raises(ValueError, match="uint8"):
        ops.frame_ingest(torch.zeros(1, 8, 8, 3), y, *args)                         # float frames
    with pytest.raises(ValueError, match="uint8"):
        ops.frame_ingest(torch.zeros(1, 8, 8, 3, dtype=torch.int8), y, *args)
    with pytest.raises(ValueError, match="3 channels"):
        ops.frame_ingest(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), y, *args)
    with pytest.raises(ValueError, match="3 channels"):
        ops.frame_ingest(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), y, *args)      # NCHW, not permuted
    with pytest.raises(ValueError, match="device"):
        ops.frame_ingest(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), y, *args)      # host frames
    meta, n = torch.zeros(4, 8), torch.zeros(1, dtype=torch.int32)
    crops = torch.zeros(4, 260, 196, 4)
    with pytest.raises(ValueError, match="uint8"):
        ops.crop_resize_u8(torch.zeros(1, 8, 8, 3), meta, n, crops)
    with pytest.raises(ValueError, match="3 channels"):
        ops.crop_resize_u8(torch.zeros(1, 8, 8, 1, dtype=torch.uint8), meta, n, crops)
    with pytest.raises(ValueError, match="device"):
        ops.crop_resize_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), meta, n, crops)
    with pytest.raises(ValueError, match="3 floats"):
        ops._f3("t", "a", (1, 2))


def test_model_entry_points_refuse_what_they_do_not_take():
    """uint8 into forward still raises, float into the uint8 entry points too (no device needed)."""
    from prpe import CombinedModel, TopDownPose
    m = CombinedModel()
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="float32"):
        m.forward(u8.permute(0, 3, 1, 2))
    for f in (m.forward_u8, m.forward_all_u8, TopDownPose(m).from_frames_u8):
        with pytest.raises(ValueError, match="uint8"):
            f(u8)                                                    # a host tensor
        with pytest.raises(ValueError, match="uint8"):
            f(torch.zeros(1, 3, 8, 8))
