"""CPU: NV12 frames in (prpe.nv12, csrc/nv12.hip) as far as the host goes -- the
integer conversion restated in numpy (``nv12_to_rgb_ref``, the yardstick tests/test_gpu_nv12.py holds
the kernels to) and held to a plain statement that shares no code with it, the coefficient tables
derived again from Kr and Kb, ``NV12Frames``' validation and views, the ABI table, every refusal of
the library before a launch, the ops wrappers' argument checks and the model's entry points.

Every comparison is an equality: the conversion is integer arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import test_facealign_host as AH
import test_faces_host as FH
import test_ingest_host as I
from prpe import FrameIngest, NV12Frames, _lib
from prpe import nv12 as N

TABLES = sorted(N.COEF)


# ------------------------------------------------------------------ the conversion, restated twice
def nv12_to_rgb_ref(y, uv, coef):
    """prpe_nv12_to_rgb in numpy int32: y [B, H, W], uv [B, ceil(H/2), ceil(W/2), 2] uint8 ->
    [B, H, W, 3] uint8 (R, G, B)."""
    y, uv = np.asarray(y), np.asarray(uv)
    B, H, W = y.shape
    y_off, cy, crv, cgu, cgv, cbu = (int(v) for v in coef)
    up = np.repeat(np.repeat(uv, 2, axis=1), 2, axis=2)[:, :H, :W].astype(np.int32)
    c = cy * (y.astype(np.int32) - y_off)
    d, e = up[..., 0] - 128, up[..., 1] - 128
    rgb = np.stack([c + crv * e + 128, c - cgu * d - cgv * e + 128, c + cbu * d + 128], axis=-1)
    return np.clip(rgb >> 8, 0, 255).astype(np.uint8)


def _plain(y, uv, coef):
    """The header's rule, pixel by pixel on Python ints with // (floor for negative numerators)."""
    B, H, W = len(y), len(y[0]), len(y[0][0])
    y_off, cy, crv, cgu, cgv, cbu = coef
    out = [[[None] * W for _ in range(H)] for _ in range(B)]
    for n in range(B):
        for i in range(H):
            for j in range(W):
                U, V = uv[n][i // 2][j // 2]
                Cc, D, E = y[n][i][j] - y_off, U - 128, V - 128
                r = (cy * Cc + crv * E + 128) // 256
                g = (cy * Cc - cgu * D - cgv * E + 128) // 256
                b = (cy * Cc + cbu * D + 128) // 256
                out[n][i][j] = [min(max(v, 0), 255) for v in (r, g, b)]
    return out


def planes(B, H, W, seed):
    """Random NV12 planes (torch uint8, host): y [B, H, W], uv [B, ceil(H/2), ceil(W/2), 2]."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (B, (H + 1) // 2, (W + 1) // 2, 2), generator=g, dtype=torch.uint8))


def nv12_sample_ref(pl, coef):
    """The converted frames of ``pl`` = (y, uv): uint8 [B, H, W, 3] (torch, host). The existing
    restatements (``ingest_ref``, ``roi_resize_ref``, ``roi_warp_ref``) apply unchanged on it."""
    y, uv = pl
    return torch.from_numpy(nv12_to_rgb_ref(y.cpu().numpy(), uv.cpu().numpy(), coef))


@pytest.mark.parametrize("key", TABLES, ids=lambda k: "-".join(k))
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 1), (1, 4, 6), (1, 3, 2)], ids=lambda s: "x".join(map(str, s)))
def test_ref_equals_the_plain_statement(key, shape):
    coef = N.COEF[key]
    y, uv = planes(*shape, seed=3)
    # the extremes in the first pixels: both clamps and negative numerators in every channel
    ext = [(0, 0, 0), (255, 255, 255), (0, 255, 0), (0, 0, 255), (255, 0, 0), (255, 255, 0), (16, 128, 128), (235, 128, 128)]
    B, H, W = shape
    for k, (Y, U, V) in enumerate(ext[:H * W]):
        i, j = divmod(k, W)
        y[0, i, j] = Y
        uv[0, i // 2, j // 2] = torch.tensor([U, V], dtype=torch.uint8)
    got = nv12_to_rgb_ref(y.numpy(), uv.numpy(), coef)
    assert got.dtype == np.uint8 and got.shape == shape + (3,)
    assert got.tolist() == _plain(y.tolist(), uv.tolist(), coef)


@pytest.mark.parametrize("key", TABLES, ids=lambda k: "-".join(k))
def test_ref_reaches_both_clamps_and_negative_numerators(key):
    """Not vacuous: over the corners of the (Y, U, V) cube each channel clamps at 0 from a negative
    numerator and at 255 from one past 255 * 256, and the neutral axis is the identity map of luma."""
    coef = N.COEF[key]
    y_off, cy, crv, cgu, cgv, cbu = coef
    corners = [(Y, U, V) for Y in (0, 255) for U in (0, 255) for V in (0, 255)]
    y = torch.tensor([[[c[0] for c in corners]]], dtype=torch.uint8)
    uv = torch.tensor([[[[c[1], c[2]] for c in corners]]], dtype=torch.uint8).repeat_interleave(1, 2)
    # one pair per pixel: a frame of width 2 * 8 whose even columns carry the corners
    yy = torch.zeros(1, 1, 16, dtype=torch.uint8)
    yy[0, 0, 0::2] = y[0, 0]
    yy[0, 0, 1::2] = y[0, 0]
    got = nv12_to_rgb_ref(yy.numpy(), uv.numpy(), coef)[0, 0, 0::2]
    nums = np.array([[cy * (Y - y_off) + crv * (V - 128) + 128, cy * (Y - y_off) - cgu * (U - 128) - cgv * (V - 128) + 128,
                      cy * (Y - y_off) + cbu * (U - 128) + 128] for Y, U, V in corners])
    for c in range(3):
        assert (nums[:, c] < 0).any() and (nums[:, c] >= 256 * 256).any()
        assert (got[nums[:, c] < 0, c] == 0).all() and (got[nums[:, c] >= 256 * 256, c] == 255).all()
    lo, hi = (16, 235) if key[1] == "limited" else (0, 255)
    grey = torch.arange(lo, hi + 1, dtype=torch.uint8).view(1, 1, -1)
    neutral = torch.full((1, 1, (grey.shape[2] + 1) // 2, 2), 128, dtype=torch.uint8)
    out = nv12_to_rgb_ref(grey.numpy(), neutral.numpy(), coef)[0, 0]
    assert (out[:, 0] == out[:, 1]).all() and (out[:, 1] == out[:, 2]).all()
    assert out[0, 0] == 0 and out[-1, 0] == 255 and (np.diff(out[:, 0].astype(int)) >= 0).all()


def test_tables_are_round_256_of_the_real_matrices():
    """Derived again in fp64 from Kr, Kb and the ranges; prpe.nv12's constants must equal it."""
    K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
    for (matrix, rng), have in N.COEF.items():
        Kr, Kb = K[matrix]
        Kg = 1.0 - Kr - Kb
        crv, cbu = 2.0 * (1.0 - Kr), 2.0 * (1.0 - Kb)
        cgu, cgv = cbu * Kb / Kg, crv * Kr / Kg
        ys, cs, y_off = (255.0 / 219.0, 255.0 / 224.0, 16) if rng == "limited" else (1.0, 1.0, 0)
        want = (y_off, round(256 * ys), round(256 * crv * cs), round(256 * cgu * cs), round(256 * cgv * cs),
                round(256 * cbu * cs))
        assert tuple(have) == want, (matrix, rng, have, want)
        assert 0 <= have[0] <= 255 and all(0 <= v <= 4096 for v in have[1:])
    assert set(N.COEF) == {(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")}
    assert N.COEF[("bt601", "limited")] == (16, 298, 409, 100, 208, 516)
    assert N.COEF[("bt709", "full")] == (0, 256, 403, 48, 120, 475)


def test_existing_restatements_apply_to_the_converted_frames():
    """``nv12_sample_ref`` hands uint8 frames [B, H, W, 3] to the restatements of the existing host
    files as they are: at equal size the ingest is rgb * a + b, a window that is the frame is the
    frame, and the identity warp too."""
    pl = planes(2, 9, 13, seed=5)
    rgb = nv12_sample_ref(pl, N.COEF[("bt709", "limited")])
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (2, 9, 13, 3)
    ing = FrameIngest(size=(9, 13), mode="stretch", norm="imagenet")
    want = rgb.double() * torch.tensor(ing.a, dtype=torch.float64) + torch.tensor(ing.b, dtype=torch.float64)
    assert torch.equal(I.ingest_ref(rgb, ing), want)
    frames64 = rgb.permute(0, 3, 1, 2).double()
    got = FH.roi_resize_ref(frames64, 1, (0.0, 0.0, 13.0, 9.0), (9, 13))
    # roi_resize_ref is grid_sample in fp64: its own rounding, 2^-40 of the 8-bit values, is all that is allowed
    assert float((got.reshape(3, 9, 13) - frames64[1]).abs().max()) <= 2.0 ** -32
    warp = AH.roi_warp_ref(rgb.permute(0, 3, 1, 2).float().contiguous(), 0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (9, 13))
    assert torch.equal(warp.reshape(3, 9, 13).double(), frames64[0])


# ------------------------------------------------------------------ NV12Frames
def test_nv12frames_views_and_validation():
    y, uv = planes(2, 7, 13, seed=1)
    f = NV12Frames(y, uv)
    assert f.shape == (2, 7, 13) and f.coef == N.COEF[("bt709", "limited")] and not f.is_cuda
    assert NV12Frames(y, uv, matrix="bt601", range="full").coef == (0, 256, 359, 88, 183, 454)
    u8 = torch.uint8
    bad = [
        (y.float(), uv), (y, uv.to(torch.int8)), (y.numpy(), uv), (y, None),                      # dtype / type
        (y[0], uv), (y[..., None], uv), (torch.zeros(0, 7, 13, dtype=u8), uv[:0]),                # y's shape
        (y, uv[:, :3]), (y, uv[:, :, :6]), (y, uv[..., :1]), (y, uv[:1]), (y, uv.reshape(2, 4, 14)),   # uv's shape
        (y.transpose(1, 2).contiguous().transpose(1, 2), uv),                                    # y's last stride is not 1
        (torch.zeros(2, 7, 26, dtype=u8)[:, :, ::2], uv),
        (y, torch.zeros(2, 4, 7, 4, dtype=u8)[..., ::2]),                                         # pairs not contiguous
        (y, torch.zeros(2, 4, 14, 2, dtype=u8)[:, :, ::2]),                                       # pair stride 4
        (y, torch.zeros(2, 4, 15, dtype=u8)[:, :, :14].unflatten(2, (7, 2))),                     # an odd chroma pitch
        (y, torch.zeros(2 * 57, dtype=u8).as_strided((2, 4, 7, 2), (57, 14, 2, 1))),              # an odd frame stride
        (y, torch.zeros(2 * 56 + 1, dtype=u8)[1:].view(2, 4, 7, 2)),                              # an odd address
    ]
    for n, (a, b) in enumerate(bad):
        with pytest.raises(ValueError):
            NV12Frames(a, b)
            pytest.fail(f"case {n} was accepted")
    with pytest.raises(ValueError, match="uv on"):
        NV12Frames(y, uv.to("meta"))                                                              # another device
    for kw in (dict(matrix="bt2020"), dict(range="tv"), dict(matrix=None)):
        with pytest.raises(ValueError):
            NV12Frames(y, uv, **kw)
    with pytest.raises(ValueError, match="channel_order"):
        f.to_rgb("gbr")
    with pytest.raises(ValueError, match="device"):
        f.to_rgb()                                                                               # host planes: refused before the ABI


def test_from_surface_aliases_the_surface():
    surf = torch.randint(0, 256, (3, 16, 20), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    f = NV12Frames.from_surface(surf, 7, 13)
    assert f.shape == (3, 7, 13) and tuple(f.uv.shape) == (3, 4, 7, 2)
    assert f.y.data_ptr() == surf.data_ptr() and f.uv.data_ptr() == surf[:, 7].data_ptr()
    assert f.y.stride() == (320, 20, 1) and f.uv.stride() == (320, 20, 2, 1)
    surf[1, 2, 5] = 201
    surf[1, 7 + 3, 2 * 6 + 1] = 77
    assert int(f.y[1, 2, 5]) == 201 and int(f.uv[1, 3, 6, 1]) == 77          # views, no copy
    g = NV12Frames.from_surface(surf, 7, 13, uv_row=8, matrix="bt601", range="full")
    assert g.uv.data_ptr() == surf[:, 8].data_ptr() and g.coef == N.COEF[("bt601", "full")]
    assert torch.equal(g.uv[0, :, :, 0], surf[0, 8:12, 0:14:2])
    NV12Frames.from_surface(surf, 8, 20, uv_row=12)                        # fills the surface exactly
    for args, kw in (((7, 13), dict(uv_row=6)), ((7, 13), dict(uv_row=0)),                 # uv_row below height
                     ((7, 13), dict(uv_row=13)), ((12, 13), {}), ((7, 21), {}),            # does not fit
                     ((0, 13), {}), ((7, 0), {})):
        with pytest.raises(ValueError):
            NV12Frames.from_surface(surf, *args, **kw)
    for s in (torch.zeros(3, 16, 21, dtype=torch.uint8),                                    # an odd pitch
              torch.zeros(3, 16, 42, dtype=torch.uint8)[:, :, ::2],                         # bytes of a row not contiguous
              torch.zeros(3, 16, 20), torch.zeros(16, 20, dtype=torch.uint8), None):
        with pytest.raises(ValueError):
            NV12Frames.from_surface(s, 7, 13)


# ------------------------------------------------------------------ the ABI
NEW = {"prpe_nv12_to_rgb": 7, "prpe_frame_ingest_nv12": 12, "prpe_crop_resize_nv12": 9, "prpe_roi_resize_nv12": 10,
       "prpe_roi_warp_nv12": 11}


def test_abi_table_has_the_nv12_entry_points():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "typedef struct prpe_nv12" in header and "} prpe_nv12;" in header
    L = _lib.lib()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", bare)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    # 2 pointers, 3 int32 (+ 4 bytes of padding), 4 int64
    assert C.sizeof(_lib.NV12) == 64 and _lib.NV12.y_sn.offset == 32 and _lib.NV12.uv_sh.offset == 56
    assert L.prpe_abi_version() == 12 == _lib.ABI_VERSION
    assert re.search(r"#define\s+PRPE_ABI_VERSION\s+12\b", header)


P0 = 0x10000
GOOD = dict(y=P0, uv=P0 + 0x4000, n=2, h=9, w=13, y_sn=1024, y_sh=16, uv_sn=512, uv_sh=14)
COEF = (16, 298, 459, 55, 136, 541)


def _src(**kw):
    v = dict(GOOD, **kw)
    return _lib.NV12(v["y"], v["uv"], v["n"], v["h"], v["w"], v["y_sn"], v["y_sh"], v["uv_sn"], v["uv_sh"])


def _coef(*v):
    return (C.c_int32 * 6)(*(v or COEF))


BAD_SRC = [dict(y=None), dict(uv=None), dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(h=-3), dict(h=2 ** 24 + 1),
           dict(w=2 ** 24 + 1, y_sh=2 ** 25, uv_sh=2 ** 25), dict(y_sh=12), dict(y_sh=-16), dict(uv_sh=12),
           dict(uv=P0 + 0x4001), dict(uv_sn=511), dict(uv_sh=15)]
BAD_COEF = [(-1, 298, 459, 55, 136, 541), (256, 298, 459, 55, 136, 541)] + \
           [tuple(COEF[:k] + (v,) + COEF[k + 1:]) for k in range(1, 6) for v in (-1, 4097)]


def _refusals(call):
    """``call(src, coef)`` with the other arguments good: every cause the five entry points share."""
    assert call(None, _coef()) == -22 and call(C.byref(_src()), None) == -22
    for kw in BAD_SRC:
        assert call(C.byref(_src(**kw)), _coef()) == -22, kw
    for c in BAD_COEF:
        assert call(C.byref(_src()), _coef(*c)) == -22, c


def test_library_refuses_bad_nv12_arguments_before_launch():
    L = _lib.lib()
    p = 0x1000
    f3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    src, coef = C.byref(_src()), _coef()

    def with_(v, **kw):
        w = _lib.View(v.ptr, v.n, v.h, v.w, v.c, v.sn, v.sh, v.sw, v.sc)
        for k, val in kw.items():
            setattr(w, k, val)
        return w

    # ---- nv12_to_rgb
    _refusals(lambda s, c: L.prpe_nv12_to_rgb(s, c, 0, p, 1024, 39, None))
    assert L.prpe_nv12_to_rgb(src, coef, 0, None, 1024, 39, None) == -22        # a null out
    assert L.prpe_nv12_to_rgb(src, coef, 0, p, 1024, 38, None) == -22          # osh below 3 w
    assert L.prpe_nv12_to_rgb(src, coef, 1, p, 1024, -39, None) == -22
    # ---- frame_ingest_nv12: the shared causes, then prpe_frame_ingest's
    dst = _lib.View(p, 2, 16, 16, 4, 2048, 96, 4, 1)

    def ingest(s=src, c=coef, d=dst, region=(0, 0, 16, 16), a=f3, b=f3, fill=f3):
        return L.prpe_frame_ingest_nv12(s, c, C.byref(d) if d is not None else None, *region, a, b, fill, None, None)
    _refusals(lambda s, c: ingest(s=s, c=c))
    assert ingest(d=None) == -22 and ingest(a=None) == -22 and ingest(b=None) == -22 and ingest(fill=None) == -22
    assert ingest(d=with_(dst, ptr=None)) == -22
    assert ingest(s=C.byref(_src(n=1))) == -22 and ingest(s=C.byref(_src(n=3))) == -22       # n != y->n
    for region in ((0, 0, 0, 16), (0, 0, 16, 0), (-1, 0, 16, 16), (0, -1, 16, 16), (1, 0, 16, 16), (0, 1, 16, 16),
                   (0, 0, 17, 16), (4, 4, 8, 13), (2 ** 31 - 1, 0, 2, 16)):
        assert ingest(region=region) == -22, region
    assert ingest(d=with_(dst, c=3)) == -22 and ingest(d=with_(dst, sc=2)) == -22 and ingest(d=with_(dst, sw=6)) == -22
    assert ingest(d=with_(dst, sh=98)) == -22 and ingest(d=with_(dst, sn=2050)) == -22
    assert ingest(d=with_(dst, ptr=p + 4)) == -22 and ingest(d=with_(dst, h=0)) == -22 and ingest(d=with_(dst, w=-3)) == -22
    assert ingest(s=C.byref(_src(n=2 ** 10)), d=with_(dst, h=2 ** 30, w=2 ** 20, n=2 ** 10),
                  region=(0, 0, 1, 1)) == -22                                   # a grid past 31 bits
    # ---- crop_resize_nv12: prpe_crop_resize_u8's
    def crop(s=src, c=coef, meta=p, n=p, max_crops=4, a=f3, b=f3, crops=p):
        return L.prpe_crop_resize_nv12(s, c, meta, n, max_crops, a, b, crops, None)
    _refusals(lambda s, c: crop(s=s, c=c))
    assert crop(meta=None) == -22 and crop(n=None) == -22 and crop(a=None) == -22 and crop(b=None) == -22
    assert crop(crops=None) == -22 and crop(crops=p + 8) == -22
    assert crop(max_crops=0) == -22 and crop(max_crops=-2) == -22 and crop(max_crops=2 ** 26) == -22
    # ---- roi_resize_nv12 and roi_warp_nv12: prpe_roi_resize_u8's and prpe_roi_warp_u8's
    ydst = _lib.View(p, 4, 9, 130, 4, 9 * 130 * 4, 130 * 4, 4, 1)

    def roi(s=src, c=coef, meta=p, n=p, max_crops=4, d=ydst, a=f3, b=f3, warp=None):
        d = C.byref(d) if d is not None else None
        if warp is None:
            return L.prpe_roi_resize_nv12(s, c, meta, n, max_crops, d, a, b, None, None)
        return L.prpe_roi_warp_nv12(s, c, meta, n, max_crops, warp[0], d, a, b, None, None)
    for warp in (None, (p,)):
        _refusals(lambda s, c: roi(s=s, c=c, warp=warp))
        assert roi(meta=None, warp=warp) == -22 and roi(n=None, warp=warp) == -22 and roi(d=None, warp=warp) == -22
        assert roi(a=None, warp=warp) == -22 and roi(b=None, warp=warp) == -22
        assert roi(max_crops=0, warp=warp) == -22 and roi(max_crops=3, warp=warp) == -22   # y->n != max_crops
        for kw in (dict(ptr=None), dict(c=3), dict(sc=2), dict(sw=6), dict(sh=522), dict(sn=4682), dict(ptr=p + 4),
                   dict(h=0), dict(w=0), dict(h=4097), dict(w=4097)):
            assert roi(d=with_(ydst, **kw), warp=warp) == -22, kw
    assert roi(warp=(None,)) == -22                                              # a null warp


# ------------------------------------------------------------------ the wrappers and the entry points
def test_ops_wrappers_refuse_host_tensors_and_mismatched_shapes():
    """Every check made before the C ABI raises ValueError; no device is needed to reach it."""
    from prpe import ops
    host = NV12Frames(*planes(2, 9, 13, seed=4))
    meta, n = torch.zeros(4, 8), torch.zeros(1, dtype=torch.int32)
    y4 = torch.zeros(2, 16, 16, 4)
    calls = [lambda f: ops.nv12_to_rgb(f, torch.zeros(2, 9, 13, 3, dtype=torch.uint8)),
             lambda f: ops.frame_ingest_nv12(f, y4, (0, 0, 16, 16), (1, 1, 1), (0, 0, 0)),
             lambda f: ops.crop_resize_nv12(f, meta, n, torch.zeros(4, 260, 196, 4)),
             lambda f: ops.roi_resize_nv12(f, meta, n, torch.zeros(4, 8, 8, 4)),
             lambda f: ops.roi_warp_nv12(f, meta, n, torch.zeros(4, 8), torch.zeros(4, 8, 8, 4))]
    for call in calls:
        with pytest.raises(ValueError, match="device"):
            call(host)                                                       # host planes
        for other in (torch.zeros(2, 9, 13, 3, dtype=torch.uint8), None, (host.y, host.uv)):
            with pytest.raises(ValueError, match="NV12Frames"):
                call(other)                                                  # not an NV12Frames

    # host planes that say they are on the device: the checks past the device check, which all come
    # before any pointer is handed to the library
    dev = _cuda_like(NV12Frames(*planes(2, 9, 13, seed=4)))
    with pytest.raises(ValueError, match="out must be a uint8 device tensor"):
        ops.nv12_to_rgb(dev, torch.zeros(2, 9, 13, 3, dtype=torch.uint8))    # a host out
    with pytest.raises(ValueError, match="float32 device tensor"):
        ops.frame_ingest_nv12(dev, y4, (0, 0, 16, 16), (1, 1, 1), (0, 0, 0))
    with pytest.raises(ValueError):
        ops.crop_resize_nv12(dev, meta, n, torch.zeros(4, 260, 196, 4))      # host crop_meta
    with pytest.raises(ValueError, match="crop_meta"):
        ops.crop_resize_nv12(dev, torch.zeros(4), n, torch.zeros(4, 260, 196, 4))
    with pytest.raises(ValueError, match="crop_meta"):
        ops.roi_resize_nv12(dev, torch.zeros(4), n, torch.zeros(4, 8, 8, 4))
    with pytest.raises(ValueError):
        ops.roi_warp_nv12(dev, meta, n, torch.zeros(4, 8), torch.zeros(4, 8, 8, 4))


def test_model_entry_points_take_nv12_as_far_as_the_device_check():
    """An ``NV12Frames`` passes the type checks of every uint8 entry point; host planes stop at the
    device check. A list of frames is still refused by the crop stages with today's message."""
    from prpe import CombinedModel, FaceCrops, PersonRecognition, PersonTracker, TopDownPose
    m = CombinedModel()
    host = NV12Frames(*planes(2, 9, 13, seed=6))
    pr = PersonRecognition(m, None)
    pra = PersonRecognition(m, None, align=True)
    dets, counts = torch.zeros(2, 4, 6), torch.zeros(2, dtype=torch.int32)
    entries = [m.forward_u8, m.forward_all_u8, TopDownPose(m).from_frames_u8, FaceCrops(m).from_frames_u8,
               lambda f: TopDownPose(m).from_detections_u8(f, dets, counts),
               lambda f: FaceCrops(m).from_detections_u8(f, dets, counts),
               lambda f: FaceCrops(m).enrol_u8(f, [1, 2]),
               pr.from_frames_u8, pra.from_frames_u8, lambda f: pra.enrol_u8(f, [1, 2]),
               lambda f: pra._aligned_u8(f, None, dets, counts, None),
               PersonTracker(pr).from_frames_u8]
    for f in entries:
        with pytest.raises(ValueError, match="CUDA"):
            f(host)
    for f in (TopDownPose(m).from_frames_u8, FaceCrops(m).from_frames_u8, pr.from_frames_u8):
        with pytest.raises(ValueError, match="a sequence of frames of different sizes is taken by the whole-frame"):
            f([torch.zeros(8, 8, 3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="FrameIngest"):
        m._check_input_u8(_cuda_like(host), "letterbox")
    x, ing = m._check_input_u8(_cuda_like(host), None)
    assert x.shape == (2, 9, 13) and isinstance(ing, FrameIngest)
    x, _ = m._check_input_u8(_cuda_like(host), None, sequence=True)
    assert isinstance(x, NV12Frames)


def _cuda_like(f):
    class Dev(NV12Frames):
        is_cuda = True
    g = Dev.__new__(Dev)
    g.__dict__.update(f.__dict__)
    return g
