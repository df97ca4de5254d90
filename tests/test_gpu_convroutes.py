"""GPU: every convolution kernel's writes, views and zero frames against fp64.

csrc/conv_igemm.hip (tiles 1-6 and the small-Co direct kernel), conv_glds.hip (10-12), conv_wave.hip
(21-29 per precision), conv_halo.hip (30-37 and the epilogue-GEMM form), conv_gemm.hip (40-49),
conv_splitk.hip (50), conv_bneck.hip (three kernels) and conv_stem.hip, each forced through
``prpe_conv_desc.tile`` (or its own entry point) with

* the input and the residual inside NaN-filled buffers (``dev_in``): a tap, halo column or
  descriptor load one pixel too far turns into a NaN in the output;
* the output a view of a sentinel-filled buffer (``Guarded``): dense, ``inner`` (rows, pixels and
  frames padded, 16-byte aligned: ``ylin`` = 0), ``concat`` (a channel slice of a wider dense NHWC
  buffer: pixel stride > Co, rows and frames linear, ``ylin`` = 1) or ``odd`` (nothing aligned:
  ``vec_out`` = 0); every float outside the view must still hold the sentinel afterwards;
* the values compared with an fp64 restatement (``ref_conv``), and ``y_amax[n] == max|y[n]|``.

Layouts refused (read off the ``*_eligible`` functions; each asserted as PrpeError + an untouched buffer):
  conv_wave / conv_halo / conv_glds: any view that clears ``vec_out`` (``odd`` y or residual, Co % 4);
      conv_glds also a prologue, precision 1 and precision 3; conv_halo tile 35 at precision 4.
  conv_gemm: the same, and any x, y or residual that is not pixel-linear (``inner``).
  conv_splitk: a residual, y_amax, chunk-major weights, x rows that are not dense, an unaligned y.
  conv_igemm tiles 1-6 and the small-Co kernel take every layout (scalar epilogue when ``vec_out`` = 0).
  prpe_bottleneck / prpe_stem_maxpool: x and y whose byte spans overlap, strides or bases off 16 bytes.

Tolerances (none from the code under test): precision 0 ``_tol * 2``; precision 2 1e-5 (every case
has a residual); precision 3 the yardstick of test_conv_f16_split_fp32_level_accuracy (error
relative to conv(|x|, |w|) scale at most max(3 e6, 10 e32, 2^-22)); precision 4 the operand
emulation of test_gpu_prec4 (1e-5 of sum|x_eff||w_eff|) and 2^-10 of sum|x||w| against fp64;
bottleneck 3 x the unfused error + 2^-22 max|y|. Every case prints its error and allowance.

Largest error / allowance per family, measured on the MI355X: conv_igemm 0.12, small-Co 0.02,
conv_glds 0.22 (precision 2 at K = 25088), conv_wave 0.29, conv_halo 0.22, its epilogue GEMM 0.05,
conv_gemm 0.11, conv_splitk 0.002, stem 0.21, bottleneck 0.25, zero-frame batches 0.31. No kernel
needed a change. 567 cases, 5 s on the MI355X.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from prpe import ops, pack
from prpe._lib import RES_PRE, PrpeError
from test_gpu_bneck import (_packs, _packs128, _packs_proj, _ref64, _ref64_proj, _unfused, _unfused128,
                            _unfused_proj)
from test_gpu_ops import WAVE_SHAPES, _decode_planes, _g, _tol, act_ref, frame_amax, ref_conv, rnd
from test_gpu_prec4 import _emul
from test_gpu_rowops import DEV, SENT, Guarded, dev_in, g_nhwc, in_nhwc, nhwc_layout, same_bits, to_nchw

pytestmark = pytest.mark.gpu

RATIO = {}                 # largest error / allowance per family, printed when the module ends


def note(fam, what, err, allow):
    r = err / allow if allow else 0.0
    RATIO[fam] = max(RATIO.get(fam, 0.0), r)
    print(f"\n[{fam}] {what}: err {err:.3e} allowance {allow:.3e} ratio {r:.3f}")
    return r


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    print("\nlargest error / allowance per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RATIO.items())))


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def conv_case(B, Ci, H, W, Co, k, s, p, act="gelu", pos=False, zero=False):
    """Operands (CPU, never modified) and the fp64 reference of one conv with scale, bias, a
    pre-activation residual and ``act``. pos: ReLU-ed frames of different ranges (precision 3 / 4);
    zero: frame 1 all zeros and a bias of both signs."""
    seed = 7000 + 13 * Co + 3 * k + H + (100 if pos else 0)
    x = rnd(B, Ci, H, W, seed=seed)
    if pos:
        x = torch.relu(x) * 7.0 * torch.tensor([1.0, 0.3, 40.0, 2.0, 0.05][:B]).view(B, 1, 1, 1)
    if zero:
        x[1] = 0.0
    c = SimpleNamespace(x=x, k=k, s=s, p=p, act=act, shape=(B, Ci, H, W, Co, k, s, p))
    c.w = rnd(Co, Ci, k, k, seed=seed + 1, scale=1.0 / math.sqrt(Ci * k * k))
    c.sc = torch.rand(Co, generator=_g(seed + 2)) + 0.5
    c.bi = rnd(Co, seed=seed + 3)
    c.sl = torch.rand(Co, generator=_g(seed + 4)) * 0.4
    Ho, Wo = out_hw(H, W, k, s, p)
    c.r = rnd(B, Co, Ho, Wo, seed=seed + 5)
    c.ref = ref_conv(x, c.w, s, p, act=act, scale=c.sc, bias=c.bi, slope=c.sl, res=c.r, res_mode=RES_PRE)
    return c


def planes_of(x_nchw):
    """The planes format of a CPU NCHW tensor, as a dense device NHWC tensor (written by the
    identity conv at precision 2, as the existing planes tests do)."""
    Ci = x_nchw.shape[1]
    xd = x_nchw.permute(0, 2, 3, 1).contiguous().to(DEV)
    xpl = torch.empty_like(xd)
    ops.conv2d(xd, pack.pack_conv("i", torch.eye(Ci).view(Ci, Ci, 1, 1), 1, 0, DEV), xpl, precision=2, y_planes=True)
    torch.cuda.synchronize()
    return xpl


def guarded_conv(x, w, *, stride=1, pad=0, act="none", scale=None, bias=None, slope=None, in_s=None, in_b=None,
                 res=None, precision=0, tile=0, k_order="auto", xk="dense", yk="dense", rk="inner", x_planes=False,
                 y_planes=False, amax=True, refuse=False, **extra):
    """ops.conv2d with x and the residual in NaN surrounds (layouts xk, rk), y a Guarded view
    (layout yk). Returns the Guarded, with ``.ya`` = the y_amax slots (CPU) when requested.
    refuse: the call must raise PrpeError and leave the whole buffer as it was."""
    B, Ci, H, W = x.shape
    Co, _, kh, kw_ = w.shape
    pk = pack.pack_conv("t", w, stride, pad, DEV, scale=scale, bias=bias, slope=slope, in_scale=in_s, in_bias=in_b,
                        act=act, k_order=k_order)
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw_) // stride + 1
    xv = dev_in(planes_of(x), *nhwc_layout(B, H, W, Ci, xk)) if x_planes else in_nhwc(x, xk)
    rv = in_nhwc(res, rk) if res is not None else None
    y = g_nhwc(B, Ho, Wo, Co, yk)
    ya = torch.zeros(B, device=DEV) if amax and not y_planes else None
    kw = dict(res=rv, res_mode=RES_PRE if res is not None else 0, precision=precision, tile=tile, y_amax=ya,
              x_planes=x_planes, y_planes=y_planes, **extra)
    if precision in (3, 4):
        kw["x_amax"] = frame_amax(x).to(DEV)
    if refuse:
        with pytest.raises(PrpeError):
            ops.conv2d(xv, pk, y.view, **kw)
        torch.cuda.synchronize()
        assert bool((y.buf == SENT).all())
        return None
    ops.conv2d(xv, pk, y.view, **kw)
    torch.cuda.synchronize()
    y.ya = ya.cpu() if ya is not None else None
    return y


def conv_of(c, **kw):
    return guarded_conv(c.x, c.w, stride=c.s, pad=c.p, act=c.act, scale=c.sc, bias=c.bi, slope=c.sl, res=c.r, **kw)


def common_checks(y, planes=False):
    """(b) nothing outside the view written, (c) no NaN inside, (d) y_amax exact; returns NCHW values."""
    assert y.untouched()
    if planes:
        hi, lo = _decode_planes(y.cpu())
        got = (hi + lo).permute(0, 3, 1, 2)
    else:
        got = to_nchw(y)
    assert not got.isnan().any()
    if y.ya is not None:
        assert torch.equal(y.ya, frame_amax(got))
    return got


def ref32_of(c):
    v = F.conv2d(c.x, c.w, None, c.s, c.p) * c.sc.view(1, -1, 1, 1) + c.bi.view(1, -1, 1, 1) + c.r
    return act_ref(v, c.act, c.sl)


def den_of(c):
    return F.conv2d(c.x.double().abs(), c.w.double().abs(), None, c.s, c.p) * c.sc.double().view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def yardstick(*key, **kkw):
    """precision 3: max(3 e6, 10 e32, 2^-22) relative to conv(|x|, |w|) scale, e6 from the
    precision-2 run (dense, automatic tile) and e32 from the CPU's fp32 conv of the same case."""
    c = conv_case(*key, **kkw)
    den = den_of(c).clamp_min(1e-30)
    e6 = float(((to_nchw(conv_of(c, precision=2)).double() - c.ref.double()).abs() / den).max())
    e32 = float(((ref32_of(c).double() - c.ref.double()).abs() / den).max())
    return max(3 * e6, 10 * e32, 2.0 ** -22), den


def assert_values(fam, what, c, got, precision, key=None, kkw=None, sel=slice(None)):
    """(a) the values against fp64 under the precision's rule (sel: the frames compared)."""
    d = (got.double() - c.ref.double()).abs()[sel]
    if precision == 0:
        err, allow = float(d.max()), _tol(c.x, c.w) * 2
    elif precision == 2:
        err, allow = float(d.max()), 1e-5
    elif precision == 3:
        allow, den = yardstick(*key, **kkw)
        err = float((d / den[sel]).max())
    else:
        emu, den = _emul(c.x, c.w, c.s, c.p, frame_amax(c.x), scale=c.sc, bias=c.bi, act=c.act, slope=c.sl, res=c.r,
                         res_mode=RES_PRE)
        e_emu = float(((got.double() - emu).abs() / (den + 1e-30))[sel].max())
        assert note(fam, what + " (vs operand emulation)", e_emu, 1e-5) <= 1.0
        err, allow = float((d / (den_of(c)[sel] + 1e-30)).max()), 2.0 ** -10
    assert note(fam, what, err, allow) <= 1.0, (what, err, allow)


def run_case(fam, key, precision, tile, xk, yk, rk="inner", **kw):
    """One guarded launch of conv_case(*key) and assertions (a)-(d)."""
    pos = precision in (3, 4)
    kkw = dict(act="relu" if pos else ("prelu" if precision == 2 else "gelu"), pos=pos)
    c = conv_case(*key, **kkw)
    planes_out = kw.get("y_planes", False)
    y = conv_of(c, precision=precision, tile=tile, xk=xk, yk=yk, rk=rk, **kw)
    got = common_checks(y, planes_out)
    assert_values(fam, f"{key} p{precision} tile {tile} x {xk} y {yk} r {rk} {kw or ''}", c, got, precision, key, kkw)
    return y


def refuse_case(key, precision, tile, xk, yk, rk="inner", **kw):
    pos = precision in (3, 4)
    c = conv_case(*key, act="relu" if pos else "gelu", pos=pos)
    conv_of(c, precision=precision, tile=tile, xk=xk, yk=yk, rk=rk, refuse=True, **kw)


S33 = {co: (2, 64, 9, 13, co, 3, 1, 1) for co in (96, 136, 150)}     # 117 pixels per frame: ragged M tiles
S11 = (2, 64, 13, 11, 256, 1, 1, 0)                                   # M = 286: one full + one ragged 256-row tile
HALO_A = (2, 64, 17, 19, 96, 3, 1, 1)                                 # ragged in both spatial dims
HALO_B = (2, 32, 16, 16, 256, 3, 1, 1)                                # exact tiles, one chunk, two Co tiles


# ====================================================================== 1. conv_igemm.hip, tiles 1-6
@pytest.mark.parametrize("co,yk", [(136, "inner"), (136, "concat"), (150, "inner"), (150, "concat"), (96, "dense"),
                                   (136, "odd")])
@pytest.mark.parametrize("k_order", [0, 1])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6])
def test_igemm_every_tile_writes_only_its_view(tile, precision, k_order, co, yk):
    """Co = 136: the vector epilogue (``col < p.Co`` per 16-byte chunk, the C tile staged in row
    chunks on tiles 5 / 6, ``ok[e] = rr < rows && m < p.M`` on the ragged last M tile); Co = 150
    and the ``odd`` view: the scalar epilogue (``col >= p.Co``, ``m >= p.M``, ``col * p.ysc``).
    A store past Co lands in the next pixel's padding (inner) or the neighbouring channels
    (concat), one past M in the row / frame padding; both are sentinel floats here. Refuses no
    layout."""
    xk = "inner" if (tile + k_order) & 1 else "dense"
    run_case("igemm", S33[co], precision, tile, xk, yk, k_order=k_order)


@pytest.mark.parametrize("tile,key", [(23, S33[136]), (28, S33[136]), (31, S33[136]), (10, S33[136]), (12, S33[136]),
                                      (40, S11), (47, S11)])
def test_unaligned_output_refused_by_vector_kernels_and_served_by_tile_0(tile, key):
    """A y view one float off the 16-byte grid clears ``vec_out``: conv_wave, conv_halo, conv_glds
    and conv_gemm (all ``kp.vec_out &&``) must refuse a forced tile without a store; the automatic
    choice falls back to conv_igemm's scalar epilogue and is right."""
    refuse_case(key, 0, tile, "dense", "odd")
    run_case("igemm", key, 0, 0, "inner" if key[5] == 3 else "dense", "odd")


def test_unaligned_residual_refused_by_vector_kernels():
    refuse_case(S33[136], 0, 23, "dense", "inner", rk="odd")
    run_case("igemm", S33[136], 0, 0, "dense", "inner", rk="odd")


# ====================================================================== 1. conv_wave.hip
WAVE_TILES = ([(0, t) for t in range(21, 30)] + [(2, t) for t in range(21, 28)] + [(3, t) for t in range(21, 28)] +
              [(4, t) for t in range(24, 30)] + [(0, 0), (2, 0), (3, 0), (4, 0)])
WAVE_LAYOUTS = [
    (S33[136], "inner", "inner", "inner"),     # 3x3 taps over a padded x; ylin = 0: the m -> (n, oh, ow) epilogue
    (S33[96], "dense", "concat", "concat"),    # ylin = rlin = 1: the m * ysw epilogue at a pixel stride > Co
    (S11, "dense", "concat", "inner"),         # 1x1 over a dense x: the pixel-contiguous A path; rlin = 0
    (S11, "inner", "inner", "concat"),         # 1x1 over a padded x: the fragment-lane A path
    (S11, "concat", "dense", "dense"),         # x pixel-linear at a stride > Ci (xsw >= Ci: still X11)
]


@pytest.mark.parametrize("key,xk,yk,rk", WAVE_LAYOUTS)
@pytest.mark.parametrize("precision,tile", WAVE_TILES)
def test_wave_every_tile_writes_only_its_view(precision, tile, key, xk, yk, rk):
    """Every forced tile of every precision (and the automatic choice) on 117- and 143-pixel frames:
    rows past M in the last wave tile (``m < p.M``), columns past Co = 136 / 96 in the last
    128-column tile (``cval``), frames smaller than a wave tile (the per-row frame scale of
    precision 3 / 4, ``two`` = false), both ``offs`` branches, and the A loads' row limit (rows past M
    beyond the descriptor; a NaN read shows in the value check). Refuses ``odd`` views (``vec_out``)."""
    run_case("wave", key, precision, tile, xk, yk, rk)


@pytest.mark.parametrize("tile", [23, 28])
@pytest.mark.parametrize("key,xk,yk", [(S33[136], "dense", "concat"), (S11, "inner", "dense"), (S33[96], "inner", "inner")])
def test_wave_planes_input_and_output_in_views(tile, key, xk, yk):
    """Planes input in a NaN surround, and planes output (``2 * (yo - col) + (col >> 3) * 16``) in a
    sentinel surround; the decoded value is compared. The planes output needs 32-byte pixels
    (prpe.h), which ``inner`` does not give: refused there."""
    run_case("wave", key, 0, tile, xk, "concat", "concat", x_planes=True)
    if yk == "inner":
        refuse_case(key, 0, tile, xk, yk, y_planes=True)
    else:
        run_case("wave", key, 0, tile, xk, yk, "inner", y_planes=True)


# ====================================================================== 1. conv_halo.hip
HALO_TILES = ([(0, t) for t in range(30, 38)] + [(3, t) for t in range(30, 38)] +
              [(4, t) for t in range(30, 38) if t != 35])


@pytest.mark.parametrize("key,xk,yk,rk", [(HALO_A, "inner", "inner", "inner"), (HALO_B, "dense", "concat", "concat"),
                                          (HALO_A, "concat", "dense", "inner")])
@pytest.mark.parametrize("precision,tile", HALO_TILES)
def test_halo_every_tile_writes_only_its_view(precision, tile, key, xk, yk, rk):
    """17 x 19 maps leave partial 8 x 16, 16 x 16 and 8 x 32 tiles (``oh < p.Ho && ow < p.Wo``), Co = 96
    a ragged column tile; the halo columns -1 and W of a padded x are NaN here where the kernel's
    descriptor must give 0. 16 x 16 maps: exact tiles, one chunk. Refuses ``odd`` views."""
    run_case("halo", key, precision, tile, xk, yk, rk)


@pytest.mark.parametrize("key,xk,yk", [(HALO_A, "inner", "concat"), (HALO_B, "dense", "inner")])
@pytest.mark.parametrize("tile", range(30, 38))
def test_halo_planes_input_in_a_view(tile, key, xk, yk):
    run_case("halo", key, 0, tile, xk, yk, "inner", x_planes=True)


def test_halo_tile_35_refused_at_precision_4():
    refuse_case(HALO_A, 4, 35, "dense", "inner")


@pytest.mark.parametrize("mode", ["fp32", "planes", "p3"])
@pytest.mark.parametrize("two_stage", [False, True])
@pytest.mark.parametrize("tile", [31, 32])
def test_halo_epilogue_gemm_writes_only_y2(tile, two_stage, mode):
    """prpe_conv_desc.w2 (+ w3): z goes to y2, a guarded ``inner`` view with n2 = 27 / 12 channels
    (``jn * 16 + fr < p.n2``, partial tiles), and the primary y, a guarded buffer, keeps every
    sentinel. Bounds: those of test_conv_halo_taps_epilogue / _two_stage (2^-14 of the sum of
    |products| per stage, carried through SiLU), against the chain in fp64 on the unfused output y'
    of the same conv."""
    B, Ci, H, W, Co = 2, 64, 17, 19, 96
    nmid, n3 = 40, 12
    n2 = n3 if two_stage else 27
    x = rnd(B, Ci, H, W, seed=7190)
    if mode == "p3":
        x = torch.relu(x) * 5.0
    w = rnd(Co, Ci, 3, 3, seed=7191, scale=1.0 / math.sqrt(Ci * 9))
    sc, bi = torch.rand(Co, generator=_g(7192)) + 0.5, rnd(Co, seed=7193)
    kw = dict(stride=1, pad=1, act="silu", scale=sc, bias=bi, precision=3 if mode == "p3" else 0,
              x_planes=mode == "planes", xk="inner")
    yd = to_nchw(guarded_conv(x, w, tile=31, **kw)).permute(0, 2, 3, 1).double()
    if two_stage:
        w2 = rnd(nmid, Co, seed=7194, scale=1.0 / math.sqrt(Co))
        s2, b2, w3 = torch.rand(nmid, generator=_g(7195)) + 0.5, rnd(nmid, seed=7196), rnd(n3, nmid, seed=7197)
        ex = dict(w2=w2.to(DEV), w3=w3.to(DEV), scale2=s2.to(DEV), bias2=b2.to(DEV), act2="silu")
        w2d, w3d, s2d, b2d = w2.double(), w3.double(), s2.double(), b2.double()
        u = (yd @ w2d.T) * s2d + b2d
        z1 = u * torch.sigmoid(u)
        ref = z1 @ w3d.T
        e1 = 1.1 * s2d.abs() * (yd.abs() @ w2d.abs().T) * 2.0 ** -14 + z1.abs() * 2.0 ** -20
        bound = (z1.abs() + e1) @ w3d.abs().T * 2.0 ** -14 + e1 @ w3d.abs().T
    else:
        w2 = rnd(n2, Co, seed=7194)
        ex = dict(w2=w2.to(DEV))
        ref = yd @ w2.double().T
        bound = (yd.abs() @ w2.double().abs().T) * 2.0 ** -14
    z = g_nhwc(B, H, W, n2, "inner")
    sink = guarded_conv(x, w, tile=tile, amax=False, yk="inner", y2=z.view, **ex, **kw)
    assert bool((sink.buf == SENT).all())
    assert z.untouched()
    got = z.cpu().double()
    assert torch.isfinite(got).all()
    r = float(((got - ref).abs() / bound.clamp_min(1e-30)).max())
    assert note("halo epilogue GEMM", f"tile {tile} two_stage {two_stage} {mode}", r, 1.0) <= 1.0


# ====================================================================== 1. conv_gemm.hip
@pytest.mark.parametrize("mode", ["fp32", "planes", "p3"])
@pytest.mark.parametrize("tile", [40, 41, 42, 43, 44, 45, 46, 47, 48, 49])
def test_gemm_every_tile_writes_only_its_view(tile, mode):
    """M = 286: one full and one ragged 256-row tile (three 128-row tiles on 43), frames of 143
    pixels inside a tile (precision 3: per-row frame scales). conv_gemm_eligible asks for
    pixel-linear x, y and residual (``xlin``, ``ylin``, ``rlin``): ``concat`` views run, with the
    row stride m * ysw at ysw = Co + 16; ``inner`` views of y, x or the residual must raise. 44-46 and
    48 are the priority / early-issue variants of 40 and 41 kept for A/B runs: the same tiles."""
    prec, pl = (3, False) if mode == "p3" else (0, mode == "planes")
    run_case("gemm", S11, prec, tile, "dense", "concat", "concat", x_planes=pl)
    run_case("gemm", S11, prec, tile, "concat", "concat", "dense", x_planes=pl)
    refuse_case(S11, prec, tile, "dense", "inner", "concat", x_planes=pl)
    refuse_case(S11, prec, tile, "dense", "concat", "inner", x_planes=pl)
    refuse_case(S11, prec, tile, "inner", "concat", "concat", x_planes=pl)


# ====================================================================== 1. conv_splitk.hip and the small-Co kernel
@pytest.mark.parametrize("yk", ["concat", "inner", "dense"])
def test_splitk_writes_only_its_view(yk):
    """Tile 50 on (5, 64, 7, 128): 5 frames in a 64-row tile (``m < p.M`` in both kernels), y a
    concat slice (``m * p.ysn + c`` at ysn = Co + 16). conv_splitk_eligible refuses a residual,
    y_amax, chunk-major weights, x rows that are not dense and an unaligned y."""
    B, Ci, H, Co = 5, 64, 7, 128
    x = rnd(B, Ci, H, H, seed=7210)
    w = rnd(Co, Ci, H, H, seed=7211, scale=1.0 / math.sqrt(Ci * H * H))
    sc, bi = torch.rand(Co, generator=_g(7212)) + 0.5, rnd(Co, seed=7213)
    sl = torch.rand(Co, generator=_g(7214)) * 0.3
    ins, inb = torch.rand(Ci, generator=_g(7215)) + 0.5, rnd(Ci, seed=7216)
    kw = dict(act="prelu", scale=sc, bias=bi, slope=sl, in_s=ins, in_b=inb, k_order=0, tile=50, amax=False)
    y = guarded_conv(x, w, yk=yk, **kw)
    got = common_checks(y)
    ref = ref_conv(x, w, 1, 0, act="prelu", scale=sc, bias=bi, slope=sl, in_s=ins, in_b=inb)
    xs = x * ins.view(1, -1, 1, 1) + inb.view(1, -1, 1, 1)
    assert note("splitk", f"y {yk}", float((got.double() - ref.double()).abs().max()), _tol(xs, w) * 2) <= 1.0
    if yk == "concat":
        guarded_conv(x, w, yk="odd", refuse=True, **kw)
        guarded_conv(x, w, xk="inner", yk=yk, refuse=True, **kw)
        guarded_conv(x, w, yk=yk, refuse=True, **{**kw, "amax": True})
        guarded_conv(x, w, yk=yk, res=rnd(B, Co, 1, 1, seed=7217), refuse=True, **kw)
        guarded_conv(x, w, yk=yk, refuse=True, **{**kw, "k_order": 1})


@pytest.mark.parametrize("xk,yk,rk", [("dense", "inner", "inner"), ("inner", "concat", "dense"), ("concat", "odd", "odd"),
                                      ("inner", "dense", "concat")])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("co", [1, 3, 4])
def test_smallco_direct_kernel_writes_only_its_view(co, precision, xk, yk, rk):
    """The direct kernel for Co <= 4 (1x1, tile 0): scalar stores ``yo + c * p.ysc`` with ``c >= p.Co``
    cut (the <3> instance serves Co = 2 and 3), ``m < p.M`` on the last pixel group. Co = 1 and 3
    are no 16-byte vectors: a float4 store would overwrite the pixel padding. Refuses no layout."""
    run_case("small-Co", (2, 64, 13, 11, co, 1, 1, 0), precision, 0, xk, yk, rk)


# ====================================================================== 2. conv_glds.hip
@pytest.mark.parametrize("B,Ci,H,W,Co,k,s,p", WAVE_SHAPES)
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("tile", [10, 11, 12])
def test_glds_every_tile_vs_fp64_and_bit_exact_vs_register_staged(tile, precision, B, Ci, H, W, Co, k, s, p):
    """conv_glds.hip walks K as conv_igemm's chunk-major path does (``issue``: kw, then kh, then the
    next 32-channel chunk = ``load_tile`` KM 2), splits A with the same ``split_planes<NP>`` and issues
    the MFMAs of a K-step per accumulator in the same (s, qa) order, then runs the same epilogue
    expression: bit-identical to tile 5, as its header claims. The source swizzle ``c = (lane & 7) ^
    swzA(row)``, the tap masks and the zero page are what a wrong value or a NaN (x sits in a NaN
    surround, padded rows and pixels) would expose; ``ok[e]`` / ``col < p.Co`` what a touched sentinel would."""
    key = (B, Ci, H, W, Co, k, s, p)
    yk = ("inner", "concat", "dense")[(tile + Co // 32) % 3]
    rk = "concat" if yk == "dense" else "inner"
    y = run_case("glds", key, precision, tile, "inner", yk, rk, k_order=1)
    c = conv_case(*key, act="prelu" if precision == 2 else "gelu", pos=False)
    base = conv_of(c, precision=precision, tile=5, xk="inner", yk=yk, rk=rk, k_order=1)
    assert same_bits(y.cpu(), base.cpu())
    assert torch.equal(y.ya, base.ya)


@pytest.mark.parametrize("tile", [10, 11, 12])
def test_glds_refusals(tile):
    """conv_glds_eligible: no prologue, precision 0 / 2 only (precision 3 belongs to the wave kernel)."""
    refuse_case(S33[136], 1, tile, "dense", "inner", k_order=1)
    refuse_case(S33[136], 3, tile, "dense", "inner", k_order=1)
    c = conv_case(*S33[136])
    ins, inb = torch.rand(64, generator=_g(7301)) + 0.5, rnd(64, seed=7302)
    conv_of(c, precision=0, tile=tile, k_order=1, in_s=ins, in_b=inb, yk="inner", refuse=True)


# ====================================================================== 3. fused stem + max-pool
def stem_pack(seed=7400):
    """Engine._stem_conv's pack: W'[co][kh * 32 + kw * 4 + c] = W[co, c, kh, kw], zero at kw = 7, c = 3."""
    w = rnd(64, 3, 7, 7, seed=seed, scale=1.0 / math.sqrt(147))
    wv = torch.zeros(64, 7, 8, 4)
    wv[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    sc, bi = torch.rand(64, generator=_g(seed + 1)) + 0.5, rnd(64, seed=seed + 2, scale=0.3)
    pk = pack.pack_matrix("stem", wv.reshape(64, 7 * 32), 7, 1, 32, 2, 0, DEV, scale=sc, bias=bi, act="relu", k_order=1)
    return w, sc, bi, pk


def stem_buf(x):
    """Engine.stem's zero-bordered NHWC4 buffer [N, H + 6, W + 8, 4], itself inside a NaN surround."""
    N, _, H, W = x.shape
    buf = torch.zeros(N, H + 6, W + 8, 4)
    buf[:, 3:3 + H, 3:3 + W, :3] = x.permute(0, 2, 3, 1)
    return dev_in(buf)


def stem_fused(x, pk, kind):
    N, _, H, W = x.shape
    y = g_nhwc(N, H // 4, W // 4, 64, kind)
    ya = torch.zeros(N, device=DEV)
    ops.stem_maxpool(stem_buf(x), H, W, frame_amax(x).to(DEV), pk, y.view, ya)
    torch.cuda.synchronize()
    y.ya = ya.cpu()
    return y


def stem_unfused(x, pk, precision=3):
    """prpe_conv2d's chunked stem over the NHWC4 view (+ its y_amax), as Engine._stem_conv runs it."""
    N, _, H, W = x.shape
    buf = stem_buf(x)
    v = torch.as_strided(buf, (N, H + 6, W, 32), (buf.stride(0), buf.stride(1), 4, 1), buf.storage_offset())
    ys = g_nhwc(N, H // 2, W // 2, 64)
    ya = torch.zeros(N, device=DEV)
    ops.conv2d(v, pk, ys.view, precision=precision, x_amax=frame_amax(x).to(DEV) if precision == 3 else None, y_amax=ya)
    torch.cuda.synchronize()
    ys.ya = ya.cpu()
    return ys


@functools.lru_cache(maxsize=None)
def stem_case(N, H, W):
    g = torch.Generator().manual_seed(H * 7 + W + N)
    x = torch.rand(N, 3, H, W, generator=g)
    x[0] *= 3.0
    w, sc, bi, pk = stem_pack()
    aff = lambda v: v * sc.to(v.dtype).view(1, -1, 1, 1) + bi.to(v.dtype).view(1, -1, 1, 1)
    full = torch.relu(aff(F.conv2d(x.double(), w.double(), None, 2, 3)))
    den = (F.conv2d(x.double().abs(), w.double().abs(), None, 2, 3) * sc.double().view(1, -1, 1, 1)).clamp_min(1e-30)
    e32 = float(((torch.relu(aff(F.conv2d(x, w, None, 2, 3))).double() - full).abs() / den).max())
    e6 = float(((to_nchw(stem_unfused(x, pk, 2)).double() - full).abs() / den).max())
    return SimpleNamespace(x=x, pk=pk, full=full, den=den, pooled=F.max_pool2d(full, 3, 2, 1),
                           yard=max(3 * e6, 10 * e32, 2.0 ** -22))


STEM_SHAPES = [(2, 4, 4), (1, 8, 164), (2, 12, 324), (1, 16, 160), (1, 16, 320)]


@pytest.mark.parametrize("kind", ["dense", "inner"])
@pytest.mark.parametrize("N,H,W", STEM_SHAPES)
def test_stem_maxpool_vs_unfused_and_fp64_in_views(N, H, W, kind):
    """Hp = Wp = 1 (the in-loop ``load_rows(py + 1)`` never runs; ``pout`` holds for one thread group),
    Wp = 41 (a second strip of one pooled column: ``px0 + pj < p.Wp``, stem columns past Ws stored as
    zeros), Wp = 81 (three strips), one and two exact strips. (a) bit-identical to prpe_conv2d's
    chunked stem + prpe_maxpool, y_amax included; (b) against fp64 conv -> affine -> relu -> max-pool:
    a full-resolution bound err <= B den carries to err <= B maxpool(den) after the pool, B the
    precision-3 yardstick measured on the full-resolution map; (c) the strided y keeps its padding.
    The unfused precision-3 stem itself is held to the same yardstick at full resolution."""
    c = stem_case(N, H, W)
    y = stem_fused(c.x, c.pk, kind)
    got = common_checks(y)
    ys = stem_unfused(c.x, c.pk)
    full = common_checks(ys)
    yu = ops.maxpool(ys.view, torch.empty(N, H // 4, W // 4, 64, device=DEV), 3, 2, 1)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), yu.cpu())
    assert torch.equal(y.ya, ys.ya)
    e_full = float(((full.double() - c.full).abs() / c.den).max())
    assert note("stem", f"unfused p3 {(N, H, W)}", e_full, c.yard) <= 1.0
    e_pool = float(((got.double() - c.pooled).abs() / F.max_pool2d(c.den, 3, 2, 1)).max())
    assert note("stem", f"fused {(N, H, W)} y {kind}", e_pool, c.yard) <= 1.0


def test_stem_maxpool_refuses_overlap_and_unaligned_y():
    c = stem_case(2, 4, 4)
    buf = stem_buf(c.x)
    xa = frame_amax(c.x).to(DEV)
    y = g_nhwc(2, 1, 1, 64, "odd")
    with pytest.raises(PrpeError):
        ops.stem_maxpool(buf, 4, 4, xa, c.pk, y.view)
    with pytest.raises(PrpeError):                          # y inside the frames' span
        ops.stem_maxpool(buf, 4, 4, xa, c.pk, torch.as_strided(buf, (2, 1, 1, 64), (buf.stride(0), 64, 64, 1),
                                                               buf.storage_offset()))
    torch.cuda.synchronize()
    assert bool((y.buf == SENT).all())


# ====================================================================== 4. all-zero frames
ZKEY33, ZKEYH, ZKEY11 = (3, 64, 9, 13, 96, 3, 1, 1), (3, 64, 17, 19, 96, 3, 1, 1), (3, 64, 13, 11, 256, 1, 1, 0)
ZERO_ROUTES = ([(ZKEY33, p, t) for p in (3, 4) for t in (0, 25, 27)] + [(ZKEY11, p, t) for p in (3, 4) for t in (0, 25, 27)] +
               [(ZKEY33, 3, 23), (ZKEY11, 3, 23)] + [(ZKEYH, p, t) for p in (3, 4) for t in (31, 34, 36)] +
               [(ZKEY11, 3, 40)])


@pytest.mark.parametrize("key,precision,tile", ZERO_ROUTES)
def test_zero_frame_is_exact_and_leaves_its_batch_mates_alone(key, precision, tile):
    """Frame 1 of 3 all zeros, x_amax[1] = 0: ``f16_scale_exp(0)`` takes e = 15 (scale 1), every
    product is 0, so y[1] = relu(bias + res) as fp32 torch evaluates it, bit for bit, and
    y_amax[1] its maximum (``amax_commit`` skips m <= 0 only when that maximum is 0). A scale
    derived from log2(0), or one frame's scale applied to its neighbour's rows in a tile that
    straddles frames (117 / 143-pixel frames), breaks frame 1 or the bit identity of frames 0 and 2
    with the two-frame launch."""
    kkw = dict(act="relu", pos=True, zero=True)
    c = conv_case(*key, **kkw)
    assert float(frame_amax(c.x)[1]) == 0.0 and bool((c.bi > 0).any()) and bool((c.bi < 0).any())
    yk = "concat" if tile >= 40 else ("inner", "concat")[tile & 1]     # (conv_gemm refuses inner views)
    rk = "concat" if key[5] == 1 else "inner"
    y = conv_of(c, precision=precision, tile=tile, xk="dense", yk=yk, rk=rk)
    got = common_checks(y)
    assert torch.isfinite(got).all()
    assert torch.equal(got[1], torch.relu(c.bi.view(-1, 1, 1) + c.r[1]))
    assert float(y.ya[1]) == float(got[1].abs().max())
    two = guarded_conv(c.x[[0, 2]], c.w, stride=c.s, pad=c.p, act=c.act, scale=c.sc, bias=c.bi, res=c.r[[0, 2]],
                       precision=precision, tile=tile, xk="dense", yk=yk, rk=rk)
    assert torch.equal(got[[0, 2]], common_checks(two))
    assert torch.equal(y.ya[[0, 2]], two.ya)
    # frames 0 and 2 against fp64 (frame 1 is exact above; its conv(|x|, |w|) is 0)
    assert_values("zero frame", f"{key} p{precision} tile {tile}", c, got, precision, key, kkw, sel=[0, 2])


def test_wave_tile_23_does_not_exist_at_precision_4():
    """conv_wave_launch has no 256 x 128 single-plane tile (it spills): 23 is refused, not remapped."""
    refuse_case(ZKEY33, 4, 23, "dense", "inner")


BNECK = {"id64": (_packs, _ref64, _unfused, 256), "proj": (_packs_proj, _ref64_proj, _unfused_proj, 64),
         "id128": (_packs128, _ref64, _unfused128, 512)}


def bneck_packs(kind, neg12=False):
    """The packs of test_gpu_bneck; neg12: BN shifts of conv1 and conv2 made <= 0 (see the zero-frame test)."""
    ws, bn, packs = BNECK[kind][0](7500)
    if neg12:
        bn = [(bn[0][0], -bn[0][1].abs()), (bn[1][0], -bn[1][1].abs())] + list(bn[2:])
        p1 = pack.pack_conv("c1", ws[0], 1, 0, DEV, scale=bn[0][0], bias=bn[0][1], act="relu")
        p2 = pack.pack_conv("c2", ws[1], 1, 1, DEV, scale=bn[1][0], bias=bn[1][1], act="relu")
        packs = (p1, p2, packs[2])
    return ws, bn, packs


def bneck_x(kind, N, H, W, zero=False):
    x = torch.relu(torch.randn(N, H, W, BNECK[kind][3], generator=_g(7510 + N + H))) * 2.0
    if zero:
        x[1] = 0.0
    return x


def bneck_run(kind, x, packs, xk="dense", yk="dense"):
    N, H, W, _ = x.shape
    xv = dev_in(x, *nhwc_layout(*x.shape, xk))
    y = g_nhwc(N, H, W, 4 * packs[0].co, yk)
    ya = torch.zeros(N, device=DEV)
    ops.bottleneck(xv, packs, y.view, x.abs().flatten(1).amax(1).to(DEV), ya)
    torch.cuda.synchronize()
    assert y.untouched()
    got = y.cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(ya.cpu(), got.abs().flatten(1).amax(1))
    return got, ya.cpu()


def bneck_bound(kind, what, x, ws, bn, packs, got):
    """test_gpu_bneck's bound: max|y - fp64| <= 3 x the unfused path's own error + 2^-22 max|y|."""
    ref = BNECK[kind][1](x, ws, bn)
    yu = BNECK[kind][2](x.to(DEV), x.abs().flatten(1).amax(1).to(DEV), packs)
    torch.cuda.synchronize()
    e_f = float((got.double() - ref).abs().max())
    e_u = float((yu.cpu().double() - ref).abs().max())
    assert note("bottleneck", what, e_f, 3 * e_u + 2.0 ** -22 * float(ref.abs().max())) <= 1.0


@pytest.mark.parametrize("neg12", [True, False])
@pytest.mark.parametrize("kind", ["id64", "proj", "id128"])
def test_bottleneck_zero_frame(kind, neg12):
    """Frame 1 of 3 all zeros (x_amax[1] = 0; conv_bneck's per-tile ``ymax = 0`` scale of t1 / t2).
    With BN shifts of both signs t1 = relu(b1) is a non-zero constant map, so conv2 of it is not
    zero and no fp32 closed form exists: that run is held to the fp64 bound. The exact statement
    needs b1, b2 <= 0 (t1 = t2 = 0 exactly): then the three epilogues chain to y[1] = relu(b3 + x[1])
    = relu(b3) bit for bit (b3 of both signs; for the projection block the pack's b3 + bd).
    Either way frames 0 and 2 equal the two-frame launch bit for bit and y_amax is exact."""
    ws, bn, packs = bneck_packs(kind, neg12)
    x = bneck_x(kind, 3, 17, 9, zero=True)
    got, ya = bneck_run(kind, x, packs, "inner", "inner")
    two, ya2 = bneck_run(kind, x[[0, 2]].contiguous(), packs, "inner", "inner")
    assert torch.equal(got[[0, 2]], two) and torch.equal(ya[[0, 2]], ya2)
    b3 = packs[2].bias.cpu()
    assert bool((b3 > 0).any()) and bool((b3 < 0).any())
    if neg12:
        assert torch.equal(got[1], torch.relu(b3).expand(17, 9, -1))
        assert float(ya[1]) == float(torch.relu(b3).max())
    bneck_bound(kind, f"{kind} zero frame neg12 {neg12}", x, ws, bn, packs, got)


@pytest.mark.parametrize("N,H,W", [(3, 8, 164), (3, 4, 4)])
def test_stem_maxpool_zero_frame(N, H, W):
    """Frame 1 all zeros: every stem value is relu(bias) (``fmaf(0 * inv, sc, bi)``), and so is every
    pooled one; y_amax[1] = max relu(bias); frames 0 and 2 as in the two-frame launch."""
    g = torch.Generator().manual_seed(7600 + W)
    x = torch.rand(N, 3, H, W, generator=g)
    x[1] = 0.0
    _, _, bi, pk = stem_pack()
    assert bool((bi > 0).any()) and bool((bi < 0).any())
    y = stem_fused(x, pk, "inner")
    got = common_checks(y)
    assert torch.isfinite(got).all()
    assert torch.equal(got[1], torch.relu(bi).view(-1, 1, 1).expand(-1, H // 4, W // 4))
    assert float(y.ya[1]) == float(torch.relu(bi).max())
    two = stem_fused(x[[0, 2]], pk, "inner")
    assert torch.equal(got[[0, 2]], common_checks(two)) and torch.equal(y.ya[[0, 2]], two.ya)


# ====================================================================== 5. bottleneck views
@pytest.mark.parametrize("yk", ["inner", "concat"])
@pytest.mark.parametrize("kind", ["id64", "proj", "id128"])
def test_bottleneck_views_bit_identical_to_dense(kind, yk):
    """(2, 17, 9): three 8-row tiles with one valid row in the last, 9 of 16 columns valid. x with
    padded rows and pixels in a NaN surround (the haloed phase-1 loads and the residual re-read go
    through ``xsh`` / ``xsw`` descriptors with BL_OOB for pixels outside the frame), y padded or a
    concat slice (``yvo`` from ``ysh`` / ``ysw``, ``ovq`` for pixels outside): bit-identical to the dense
    launch, nothing outside the view written, and within test_gpu_bneck's fp64 bound."""
    ws, bn, packs = bneck_packs(kind)
    x = bneck_x(kind, 2, 17, 9)
    dense, ya_d = bneck_run(kind, x, packs)
    got, ya = bneck_run(kind, x, packs, "inner", yk)
    assert torch.equal(got, dense) and torch.equal(ya, ya_d)
    bneck_bound(kind, f"{kind} x inner y {yk}", x, ws, bn, packs, got)


@pytest.mark.parametrize("kind", ["id64", "proj", "id128"])
def test_bottleneck_refuses_overlapping_views(kind):
    """``views_overlap``: in place (identity blocks), and x a channel slice of the buffer y fills."""
    _, _, packs = bneck_packs(kind)
    cin, cout = BNECK[kind][3], 4 * packs[0].co
    big = Guarded((1, 8, 8, cout + cin))
    xa = torch.ones(1, device=DEV)
    with pytest.raises(PrpeError):
        ops.bottleneck(big.view[..., cout:], packs, big.view[..., :cout], xa)
    if cin == cout:
        with pytest.raises(PrpeError):
            ops.bottleneck(big.view[..., :cout], packs, big.view[..., :cout], xa)
    torch.cuda.synchronize()
    assert bool((big.buf == SENT).all())
