"""CPU: the mixed-size, antialiased ingest (prpe_frame_ingest_multi) as far as the
host goes -- a numpy fp32 restatement written to the header's order of operations
(``ingest_multi_ref``, which tests/test_gpu_ingest_multi.py holds the kernel to bit for bit), a
second, plain fp64 statement that shares no code with it, both pinned to torch's own
F.interpolate(antialias=True) within an allowance derived from the number formats, the edges of the
rule, ``FrameIngest``'s new arguments, the library's refusals before launch and the checks of
``ops.frame_ingest_multi``."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from prpe import FrameIngest, _lib

f32 = np.float32
NORMS = {"raw": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), "unit": None, "imagenet": None, "half": None}


def norm_ab(name):
    """(a, b) as the fp32 values FrameIngest hands the kernel."""
    ing = FrameIngest(norm=NORMS[name] or name)
    return ing.a, ing.b


# ------------------------------------------------------------------ the fp32 restatement (header order)
def _aa_axis(S, n_out):
    """Antialias axis, scale = S / n_out > 1: per output index (lo, [w_k as fp32]), fp64 as the header says."""
    scale = S / n_out
    inv = 1.0 / scale
    out = []
    for o in range(n_out):
        centre = scale * (o + 0.5)
        lo = max(int(centre - scale + 0.5), 0)
        hi = min(int(centre + scale + 0.5), S)
        t = []
        for k in range(lo, hi):
            x = abs((k - centre + 0.5) * inv)
            t.append(1.0 - x if x < 1.0 else 0.0)
        s = 0.0
        for v in t:
            s += v
        out.append((lo, [f32(v / s) for v in t]))
    return out


def _two_tap_axis(S, n_out):
    """prpe_frame_ingest's axis: per output index (a, b, frac as fp32)."""
    scale = S / n_out
    out = []
    for o in range(n_out):
        s = min(max((o + 0.5) * scale - 0.5, 0.0), float(S - 1))
        fl = math.floor(s)
        a = int(fl)
        out.append((a, a + 1 if a + 1 < S else a, f32(s - fl)))
    return out


def ingest_multi_ref(frame, geom, a, b, fill, swap_rb, antialias, size=None):
    """prpe_frame_ingest_multi for ONE frame in numpy fp32, operation for operation as include/prpe.h
    states it: ``frame`` uint8 [Hs, Ws, 3] (source channel order), ``geom`` = (top, left, nh, nw).
    Returns the region [nh, nw, 3], or with ``size`` = (H, W) the whole interior [H, W, 4] (fill
    outside the region, channel 3 = 0)."""
    v = np.asarray(frame, dtype=np.uint8)
    if swap_rb:
        v = v[:, :, ::-1]
    v = v.astype(f32)
    Hs, Ws, _ = v.shape
    top, left, nh, nw = (int(g) for g in geom)
    a, b, fill = (np.asarray(t, dtype=f32) for t in (a, b, fill))
    h = np.zeros((Hs, nw, 3), f32)                                   # the horizontal values, per source row
    if antialias and Ws > nw:
        for j, (lo, w) in enumerate(_aa_axis(Ws, nw)):
            acc = np.zeros((Hs, 3), f32)                             # first tap + weighted differences from it
            for k, wk in enumerate(w):
                if k:
                    acc = acc + wk * (v[:, lo + k, :] - v[:, lo, :])  # fp32 product, then fp32 add
            h[:, j, :] = v[:, lo, :] + acc
    else:
        for j, (xa, xb, ax) in enumerate(_two_tap_axis(Ws, nw)):
            h[:, j, :] = v[:, xa, :] + ax * (v[:, xb, :] - v[:, xa, :])
    raw = np.zeros((nh, nw, 3), f32)
    if antialias and Hs > nh:
        for i, (lo, w) in enumerate(_aa_axis(Hs, nh)):
            acc = np.zeros((nw, 3), f32)
            for r, wr in enumerate(w):
                if r:
                    acc = acc + wr * (h[lo + r] - h[lo])
            raw[i] = h[lo] + acc
    else:
        for i, (ya, yb, ay) in enumerate(_two_tap_axis(Hs, nh)):
            raw[i] = h[ya] + ay * (h[yb] - h[ya])
    y = raw * a + b
    assert y.dtype == f32
    if size is None:
        return y
    H, W = size
    out = np.zeros((H, W, 4), f32)
    out[:, :, :3] = fill * a + b
    out[top:top + nh, left:left + nw, :3] = y
    return out


# ------------------------------------------------------------------ the plain fp64 statement (own code)
def ingest_multi_plain(frame, geom, a, b, swap_rb, antialias):
    """The same semantics said plainly in fp64, explicit loops over the taps, nothing shared with the
    restatement above (the triangle is written 1 - |k + 0.5 - centre| / scale, the two-tap axis as a
    two-entry weight list): the region [nh, nw, 3]."""
    src = np.asarray(frame).astype(np.float64)
    Hs, Ws, _ = src.shape
    _, _, nh, nw = geom

    def taps(S, n, o):
        scale = S / n
        if antialias and scale > 1:
            c = (o + 0.5) * scale
            first, last = max(int(c - scale + 0.5), 0), min(int(c + scale + 0.5), S)
            ws = [max(0.0, 1.0 - abs(k + 0.5 - c) / scale) for k in range(first, last)]
            tot = sum(ws)
            return [(k, w / tot) for k, w in zip(range(first, last), ws)]
        pos = min(max((o + 0.5) * scale - 0.5, 0.0), S - 1.0)
        k0 = int(math.floor(pos))
        return [(k0, 1.0 - (pos - k0)), (min(k0 + 1, S - 1), pos - k0)]

    out = np.zeros((nh, nw, 3))
    tx = [taps(Ws, nw, j) for j in range(nw)]
    for i in range(nh):
        for r, wr in taps(Hs, nh, i):
            for j in range(nw):
                for k, wk in tx[j]:
                    out[i, j] += wr * wk * src[r, k]
    if swap_rb:
        out = out[:, :, ::-1]
    return out * np.asarray(a, np.float64) + np.asarray(b, np.float64)


def oracle(frame, geom, a, b, swap_rb):
    """torch on the CPU, fp64: F.interpolate(antialias=True) of the raw values, then raw * a + b.
    One column into one column is asked of torch as two equal columns into two: with a width of 1
    on both sides the torch build this was written against returns its first output row in every
    row, whatever the rows hold (a [1, 3, 97, 1] tensor into (64, 1): 64 equal rows; into (64, 2), or
    from two columns, it does not); an x axis at scale 1 is the identity, so column 0 of the widened
    result is torch's rule for the frame, on a fixed torch as on this one."""
    x = torch.from_numpy(np.ascontiguousarray(frame)).permute(2, 0, 1)[None].double()
    if swap_rb:
        x = x.flip(1)
    _, _, nh, nw = geom
    if x.shape[3] == 1 and nw == 1:
        x = x.repeat(1, 1, 1, 2)
    r = F.interpolate(x, size=(nh, x.shape[3] if nw == 1 and frame.shape[1] == 1 else nw), mode="bilinear",
                      align_corners=False, antialias=True)[0].permute(1, 2, 0)[:, :nw]
    return r.numpy() * np.asarray(a, np.float64) + np.asarray(b, np.float64)


def allowance(frame_hw, geom, a, y):
    """The fp32 roundings of the restatement against an exact evaluation of the same rule. An output
    with n_x, n_y taps: the weights sum to 1 and the differences from the first tap are at most 255,
    so rounding the weights costs at most 2^-24 * 255 per axis, the products as much, the differences
    of the vertical pass as much, each of the n adds of a sum at most 2^-24 * 255 and the add of the
    first tap one more; the affine adds two roundings. Bounded by
    (n_x + n_y + 8) * 2^-24 * 255 * |a_c| + 2^-23 * |y| (a two-tap axis counts n = 2)."""
    Hs, Ws = frame_hw
    _, _, nh, nw = geom
    n_x = max(len(w) for _, w in _aa_axis(Ws, nw)) if Ws > nw else 2
    n_y = max(len(w) for _, w in _aa_axis(Hs, nh)) if Hs > nh else 2
    return (n_x + n_y + 8) * 2.0 ** -24 * 255 * np.abs(np.asarray(a, np.float64)) + 2.0 ** -23 * np.abs(y)


# ------------------------------------------------------------------ the cases (shared with the GPU file)
def frame_of(Hs, Ws, seed):
    g = np.random.default_rng(seed)
    f = g.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    f[::3, ::2] = 255                                                # fine texture: what aliases
    f[1::3, 1::2] = 0
    return f


# name: (Hs, Ws), (H, W), mode or an explicit region, norm, swap_rb
CASES = {
    "integer_2x": ((64, 96), (32, 48), "stretch", "raw", False),
    "non_integer": ((97, 131), (32, 48), "stretch", "imagenet", True),
    "letterbox_270x480": ((270, 480), (64, 64), "letterbox", "unit", False),
    "x_same_y_down": ((97, 48), (32, 48), "stretch", "half", False),          # scale exactly 1 on x
    "y_same_x_down": ((32, 131), (32, 48), "stretch", "raw", True),           # scale exactly 1 on y
    "x_same_y_up_33x64": ((33, 64), (64, 64), "stretch", "unit", False),      # no axis shrinks
    "upscale_7x5": ((7, 5), (32, 48), "letterbox", "imagenet", False),
    "one_row_out": ((7, 480), (32, 48), "letterbox", "raw", False),            # nh = 1
    "source_1x1": ((1, 1), (32, 48), "letterbox", "half", False),
    "source_1x131": ((1, 131), (32, 48), "stretch", "raw", False),             # a source side of 1
    "source_97x1": ((97, 1), (64, 64), "letterbox", "unit", True),
    "scale_32": ((1024, 33), (32, 48), "stretch", "raw", False),               # 1024 = 32 * 32 on y
    "region_top_left": ((97, 131), (32, 48), (0, 0, 9, 11), "unit", False),
    "region_bottom_right": ((97, 131), (32, 48), (32 - 13, 48 - 17, 13, 17), "imagenet", False),
    "region_inner": ((270, 480), (64, 64), (5, 7, 50, 33), "raw", True),
}


def case(name):
    (Hs, Ws), size, mode, norm, swap = CASES[name]
    geom = tuple(mode) if not isinstance(mode, str) else FrameIngest(size=size, mode=mode).geometry(Hs, Ws)
    a, b = norm_ab(norm)
    seed = sorted(CASES).index(name)
    return frame_of(Hs, Ws, seed), size, geom, a, b, (114.0, 0.0, 255.0), swap


_ref_cache = {}


def ref_of(name):
    """The restatement of a case, computed once and shared (read-only) by the tests that need it."""
    if name not in _ref_cache:
        frame, size, geom, a, b, fill, swap = case(name)
        r = ingest_multi_ref(frame, geom, a, b, fill, swap, True, size)
        r.setflags(write=False)
        _ref_cache[name] = r
    return _ref_cache[name]


# ------------------------------------------------------------------ pinned to torch, and to the plain statement
def test_restatement_is_pinned_to_torch_antialias_within_the_derived_allowance(capsys):
    worst = (0.0, None)
    for name in CASES:                                               # every case: none is left out
        frame, size, geom, a, b, fill, swap = case(name)
        top, left, nh, nw = geom
        got = ref_of(name)[top:top + nh, left:left + nw, :3].astype(np.float64)
        want = oracle(frame, geom, a, b, swap)
        ratio = float((np.abs(got - want) / allowance(frame.shape[:2], geom, a, want)).max())
        worst = max(worst, (ratio, name))
        assert ratio <= 1.0, (name, ratio)
    with capsys.disabled():
        print(f"\ningest_multi_ref vs torch antialias fp64: worst error / allowance = {worst[0]:.4f} ({worst[1]})")


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_plain_statement(name):
    frame, size, geom, a, b, fill, swap = case(name)
    top, left, nh, nw = geom
    got = ref_of(name)[top:top + nh, left:left + nw, :3].astype(np.float64)
    want = ingest_multi_plain(frame, geom, a, b, swap, True)
    assert float((np.abs(got - want) / allowance(frame.shape[:2], geom, a, want)).max()) <= 1.0


def test_fill_channel_3_and_region_placement():
    frame, size, geom, a, b, fill, swap = case("region_inner")
    r = ref_of("region_inner")
    top, left, nh, nw = geom
    fv = np.asarray(fill, f32) * np.asarray(a, f32) + np.asarray(b, f32)
    mask = np.ones(size, bool)
    mask[top:top + nh, left:left + nw] = False
    assert r.shape == size + (4,) and r.dtype == f32
    assert np.array_equal(r[mask][:, :3], np.broadcast_to(fv, (mask.sum(), 3))) and not r[..., 3].any()
    assert np.array_equal(r[top:top + nh, left:left + nw, :3], ingest_multi_ref(frame, geom, a, b, fill, swap, True))


# ------------------------------------------------------------------ the weights
@pytest.mark.parametrize("S,n", [(96, 48), (131, 48), (480, 64), (1024, 32), (33, 32), (65, 2), (7, 1), (1920, 640),
                                 (3840, 640), (2160, 360)])
def test_weights_are_non_negative_sum_to_one_and_windows_stay_inside(S, n):
    scale = S / n
    taps = _aa_axis(S, n)
    assert len(taps) == n
    for lo, w in taps:
        assert lo >= 0 and lo + len(w) <= S and 1 <= len(w) <= 2 * scale + 1
        assert all(x >= 0 for x in w) and all(x.dtype == f32 for x in w)
        assert abs(math.fsum(float(x) for x in w) - 1.0) <= 2.0 ** -22
    # the first and the last output pixel: the window is cut at the frame's edge, so it is shorter
    # than an interior one and its weights are renormalised over what is left
    inner = max(len(w) for _, w in taps)
    if n > 2 and scale >= 2:
        assert len(taps[0][1]) < inner and len(taps[-1][1]) < inner
    assert taps[0][0] == 0 and taps[-1][0] + len(taps[-1][1]) == S


def test_weights_are_torchs_to_the_bit():
    """An identity image through torch's fp64 antialias gives torch's weights: aten forms
    (k - centre + 0.5) * (1 / scale), which the header states; rounded to fp32 they are the kernel's."""
    for S, n in ((33, 5), (131, 48), (1024, 32), (65, 2)):
        eye = torch.eye(S, dtype=torch.float64)[None, None]
        w = F.interpolate(eye, size=(S, n), mode="bilinear", align_corners=False, antialias=True)[0, 0].numpy()
        for j, (lo, ws) in enumerate(_aa_axis(S, n)):
            col = np.zeros(S)
            col[lo:lo + len(ws)] = ws
            assert np.array_equal(col.astype(f32), w[:, j].astype(f32)), (S, n, j)


def test_scale_32_is_the_limit():
    assert max(len(w) for _, w in _aa_axis(1024, 32)) <= 2 * 32 + 1
    from prpe import ops
    assert ops.INGEST_MAX_SCALE == 32


# ------------------------------------------------------------------ bilinear where no axis shrinks
@pytest.mark.parametrize("name", ["x_same_y_up_33x64", "upscale_7x5", "source_1x1"])
def test_antialias_is_the_bilinear_restatement_when_no_axis_is_downscaled(name):
    frame, size, geom, a, b, fill, swap = case(name)
    assert frame.shape[0] <= geom[2] and frame.shape[1] <= geom[3]
    assert np.array_equal(ref_of(name), ingest_multi_ref(frame, geom, a, b, fill, swap, False, size))


def test_bilinear_restatement_is_prpe_frame_ingests():
    """filter 0 restates prpe_frame_ingest: against torch's own antialias=False in fp64, and at
    equal size the bits of u8.float() * a + b."""
    for name in ("non_integer", "upscale_7x5", "letterbox_270x480"):
        frame, size, geom, a, b, fill, swap = case(name)
        got = ingest_multi_ref(frame, geom, a, b, fill, swap, False).astype(np.float64)
        x = torch.from_numpy(frame.copy()).permute(2, 0, 1)[None].double()
        x = x.flip(1) if swap else x
        want = F.interpolate(x, size=geom[2:], mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
        want = want * np.asarray(a, np.float64) + np.asarray(b, np.float64)
        assert float((np.abs(got - want) / allowance((1, 1), geom, a, want)).max()) <= 1.0
    frame = frame_of(32, 48, 99)
    a, b = norm_ab("imagenet")
    for aa in (False, True):
        got = ingest_multi_ref(frame, (0, 0, 32, 48), a, b, (0, 0, 0), False, aa)
        want = torch.from_numpy(frame.copy()).float() * torch.tensor(a) + torch.tensor(b)
        assert np.array_equal(got, want.numpy())


def test_constant_frames_stay_constant():
    """All-zero and all-255 frames give exactly b and 255 * a + b at every scale: a sum is its first
    tap plus weighted differences from it, so what the rounded weights sum to never enters."""
    a, b = norm_ab("imagenet")
    for Hs, Ws in ((64, 96), (97, 131), (1024, 33), (270, 480), (7, 480)):
        for val in (0, 255):
            frame = np.full((Hs, Ws, 3), val, np.uint8)
            got = ingest_multi_ref(frame, (0, 0, 32, 48), a, b, (0, 0, 0), False, True)
            want = f32(val) * np.asarray(a, f32) + np.asarray(b, f32)
            assert np.array_equal(got, np.broadcast_to(want, got.shape)), (Hs, Ws, val)


# ------------------------------------------------------------------ FrameIngest
def test_frame_ingest_without_the_keyword_is_unchanged():
    ing = FrameIngest()
    assert ing.antialias is False
    assert repr(ing) == (f"FrameIngest(size=(640, 640), mode='letterbox', a={ing.a}, b={ing.b}, "
                         f"channel_order='rgb', fill=(114.0, 114.0, 114.0))")
    assert sorted(vars(ing)) == ["a", "antialias", "b", "channel_order", "fill", "mode", "size"]
    aa = FrameIngest(size=(32, 48), mode="stretch", norm="half", antialias=True)
    assert aa.antialias is True and repr(aa).endswith(", antialias=True)")
    assert repr(aa).replace(", antialias=True", "") == repr(FrameIngest(size=(32, 48), mode="stretch", norm="half"))
    assert aa.geometry(97, 131) == FrameIngest(size=(32, 48), mode="stretch").geometry(97, 131)


def test_geometry_batch_is_geometry_per_row():
    ing = FrameIngest(size=(640, 640))
    sizes = [(720, 1280), (1080, 1920), (2160, 3840), (1920, 1080), (7, 5), (1, 5000)]
    g = ing.geometry_batch(sizes)
    assert g.shape == (6, 4) and g.dtype == torch.int32 and g.device.type == "cpu"
    assert [tuple(r) for r in g.tolist()] == [ing.geometry(*s) for s in sizes]
    assert torch.equal(ing.geometry_batch(torch.tensor(sizes)), g)
    for bad in ([], [(1, 2, 3)], [(0, 4)]):
        with pytest.raises(ValueError):
            ing.geometry_batch(bad)


def test_to_source_and_to_model_per_frame():
    ing = FrameIngest(size=(640, 640))
    sizes = [(720, 1280), (1080, 1920), (2160, 3840), (1920, 1080)]
    g = torch.Generator().manual_seed(5)
    p = torch.rand(4, 6, 4, generator=g) * 640
    src = ing.to_source(p, sizes)
    assert src.shape == p.shape and src.dtype == p.dtype
    for n, (Hs, Ws) in enumerate(sizes):
        one = ing.to_source(p[n], Hs, Ws)
        assert float((src[n] - one).abs().max()) <= 4 * max(Hs, Ws) * 2.0 ** -24
        back = ing.to_model(src, sizes)[n]                           # the round trip, per frame
        assert float((back - p[n]).abs().max()) <= 8 * 640 * 2.0 ** -24
        assert float((ing.to_model(src, torch.tensor(sizes))[n] - back).abs().max()) == 0.0
    pts = p[:, 0, :2]                                                # [B, 2]: one point per frame
    assert torch.equal(ing.to_source(pts, sizes), src[:, 0, :2])
    with pytest.raises(ValueError):
        ing.to_source(p[:3], sizes)                                  # 3 rows for 4 sizes
    with pytest.raises(ValueError):
        ing.to_source(torch.zeros(4, 3), sizes)


# ------------------------------------------------------------------ the library's refusals
def _table(*rows):
    t = (_lib.IngestSrc * len(rows))()
    for n, r in enumerate(rows):
        t[n] = _lib.IngestSrc(*r)
    return t


def test_abi_table_has_the_multi_entry_point():
    import os
    import re
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    decl = re.search(r"\bint prpe_frame_ingest_multi\s*\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert decl and "typedef struct prpe_ingest_src" in header
    assert len(decl.group(1).split(",")) == 10 == len(_lib.SIGNATURES["prpe_frame_ingest_multi"][1])
    assert C.sizeof(_lib.IngestSrc) == 56 and hasattr(_lib.lib(), "prpe_frame_ingest_multi")
    assert _lib.lib().prpe_abi_version() == 12


def test_library_refuses_bad_multi_arguments_before_launch():
    L = _lib.lib()
    p = 0x1000
    f3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    good = (p, 8, 10, 30, 3, 1, 0, 0, 16, 16)                        # ptr, h, w, sh, sw, sc, top, left, nh, nw
    dst = _lib.View(p, 2, 16, 16, 4, 2048, 96, 4, 1)

    def call(rows=(good, good), B=2, d=dst, filt=0, a=f3, b=f3, fill=f3, table=True):
        return L.prpe_frame_ingest_multi(_table(*rows) if table else None, B, C.byref(d) if d is not None else None,
                                         filt, a, b, fill, 0, None, None)

    def row(**kw):
        names = ("ptr", "h", "w", "sh", "sw", "sc", "top", "left", "nh", "nw")
        return tuple(kw.get(k, v) for k, v in zip(names, good))

    def with_(v, **kw):
        w = _lib.View(v.ptr, v.n, v.h, v.w, v.c, v.sn, v.sh, v.sw, v.sc)
        for k, val in kw.items():
            setattr(w, k, val)
        return w

    assert call(table=False) == -22 and call(d=None) == -22          # null pointers
    assert call(a=None) == -22 and call(b=None) == -22 and call(fill=None) == -22
    assert call(d=with_(dst, ptr=None)) == -22
    assert call(B=0) == -22 and call(B=-1) == -22                    # B < 1
    assert call(rows=(good,), B=1) == -22                            # B != y->n
    assert call(rows=(good,) * 3, B=3) == -22
    assert call(filt=2) == -22 and call(filt=-1) == -22              # filter outside {0, 1}
    for bad in (row(ptr=None), row(h=0), row(w=0), row(h=-4), row(h=2 ** 24 + 1), row(w=2 ** 24 + 1)):
        assert call(rows=(good, bad)) == -22 and call(rows=(bad, good), filt=1) == -22, bad
    for region in ((0, 0, 0, 16), (0, 0, 16, 0), (-1, 0, 16, 16), (0, -1, 16, 16), (1, 0, 16, 16), (0, 1, 16, 16),
                   (0, 0, 17, 16), (4, 4, 8, 13), (2 ** 31 - 1, 0, 2, 16)):
        bad = row(top=region[0], left=region[1], nh=region[2], nw=region[3])
        assert call(rows=(good, bad)) == -22, region                 # empty, or not inside H x W
    # filter 1: an axis shrinks by at most 32 -- 16 * 32 + 1 rows or columns into 16 are refused
    over_h, over_w = row(h=16 * 32 + 1), row(w=16 * 32 + 1)
    assert call(rows=(good, over_h), filt=1) == -22 and call(rows=(over_w, good), filt=1) == -22
    assert call(rows=(good, row(h=2, nh=1, w=65, nw=2)), filt=1) == -22
    # prpe_frame_ingest's conditions on y
    assert call(d=with_(dst, c=3)) == -22 and call(d=with_(dst, sc=2)) == -22
    assert call(d=with_(dst, sw=6)) == -22 and call(d=with_(dst, sh=98)) == -22 and call(d=with_(dst, sn=2050)) == -22
    assert call(d=with_(dst, ptr=p + 4)) == -22 and call(d=with_(dst, h=0)) == -22 and call(d=with_(dst, w=-3)) == -22
    assert call(d=with_(dst, h=2 ** 30, w=2 ** 20), rows=(row(nh=1), row(nh=1))) == -22    # a grid past 31 bits


def test_ops_validate_multi_arguments_before_any_launch():
    from prpe import ops
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    y = torch.zeros(2, 8, 8, 4)
    g = [(0, 0, 8, 8)] * 2
    ab = ((1, 1, 1), (0, 0, 0))
    with pytest.raises(ValueError, match="no frames"):
        ops.frame_ingest_multi([], y, [], 0, *ab)
    with pytest.raises(ValueError, match="uint8"):
        ops.frame_ingest_multi([u8(8, 8, 3), torch.zeros(8, 8, 3)], y, g, 0, *ab)
    with pytest.raises(ValueError, match="3 channels"):
        ops.frame_ingest_multi([u8(8, 8, 3), u8(3, 8, 8)], y, g, 0, *ab)
    with pytest.raises(ValueError, match="3 channels"):
        ops.frame_ingest_multi([u8(8, 8, 3), u8(0, 8, 3)], y, g, 0, *ab)
    with pytest.raises(ValueError, match="filter"):
        ops.frame_ingest_multi(u8(2, 8, 8, 3), y, g, 2, *ab)         # a 4-D tensor is taken as its frames
    with pytest.raises(ValueError, match="regions"):
        ops.frame_ingest_multi(u8(2, 8, 8, 3), y, g[:1], 0, *ab)
    with pytest.raises(ValueError, match="regions"):
        ops.frame_ingest_multi(u8(2, 8, 8, 3), y, [(0, 0, 8), (0, 0, 8)], 0, *ab)
    with pytest.raises(ValueError, match="device"):
        ops.frame_ingest_multi(u8(2, 8, 8, 3), y, g, 1, *ab)         # a host destination


def test_model_entry_points_take_sequences_only_where_the_ingest_is_whole_frame():
    """The crop stages resample from one source tensor: a sequence passed to them is refused with a
    ValueError that says so; the whole-frame entry points get as far as the device check."""
    from prpe import CombinedModel, TopDownPose
    m = CombinedModel()
    seq = [torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(6, 9, 3, dtype=torch.uint8)]
    aa = FrameIngest(antialias=True)
    for f in (m.forward_u8, m.forward_all_u8):
        with pytest.raises(ValueError, match=r"sequence of uint8 CUDA\(HIP\) frames"):
            f(seq, aa)                                               # host tensors
        with pytest.raises(ValueError, match="sequence"):
            f([])
    for f in (TopDownPose(m).from_frames_u8,):
        with pytest.raises(ValueError, match="whole-frame ingest only"):
            f(seq)
