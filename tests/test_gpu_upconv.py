"""GPU: every prpe_upconv3x3 kernel (csrc/pointwise.hip) at every dispatch branch against fp64.

Stage 2 of the upsample o conv3x3 rewrite: ``upconv_fused_kernel<VW, ACT>``, ``upconv_dma_kernel<ACT, PL>``,
``upconv_unit_kernel<CO>`` and the separable pair ``upconv_h_kernel`` / ``upconv_out_kernel``.

The reference (``upconv_ref``) restates stage 2 on ``z`` itself in plain torch on the CPU (``F.interpolate`` of
the 9 Co tap maps, ``F.pad`` + nine shifted slices, scale / bias, ``act_ref``), so the tap GEMM and its bf16
noise stay out of the comparison. It shares nothing with ``bilin_src``; ``test_reference_hand_case`` (no GPU)
pins its tap order ``(3 dy + dx) Co + c`` and the shift direction on written-out numbers.

Harness of every case (``run``): z sits in a NaN-filled buffer (``dev_in``): a load one pixel, row, tap or frame
too far is a NaN in the output. The dense z's buffer ends ``MARGIN`` floats after the view's last float, which is
what the DMA descriptor bound ``zbytes`` must respect; the padded z layouts enter ``dvo`` and ``zbytes``. y is a
``Guarded`` view: every float outside it holds the sentinel afterwards, a skipped element inside it fails the value
check. No case is exempt from the value check; every case prints err / allowance.

Tolerances (none taken from the kernels)
  allowance = 4 e_ref, e_ref = max |float32 ``upconv_ref`` - float64 ``upconv_ref``| over the case's whole output
      (the ``scaled_tol`` convention of test_gpu_rowops; 4 covers another legitimate fp32 summation order).
  A case with fewer than 4096 outputs borrows e_ref from a named larger case with the same data scale, activation
      and operands present: ``YARD_UNIT`` (2 x 33 x 65, Co 3, output grid = input grid, align_corners) for the
      unit-scale geometry, ``YARD_GEN`` (2 x 7 x 9 -> 20 x 13, Co 24, align_corners=False) for every other.
  SiLU, sigmoid and GELU add what test_epilogue_activation_accuracy grants the hardware exp2 / erf forms:
      4 ulp of |ref| + 1e-35, plus 2^-22 |v| of the pre-activation v for GELU.
  Bit equality on finite z, asserted in addition: every one-pass result == the separable result of the same
      operands (``sep_bits``), DMA == fused == separable (``fused_bits``: the same operands through an NCHW y, which
      the DMA route refuses), unit == separable. pointwise.hip promises it (lerp_add, lerp_add2).
  y_amax: the slot holds the bits of max|y[n]| over the view; a slot that already holds more keeps it; the
      floats beside the slots stay.
  Planes: hi == RNE_bf16(v), lo == RNE_bf16(v - hi), v = the same route's fp32 output of the same case, which
      is itself held to fp64.
  Data: z uniform in [-1, 1] (``rnd``); one case per route with z (and the bias) scaled by 50 and by 1e-3.

Routes. The library does not say which kernel ran. ``route_of`` is a restatement of HOST code (prpe_upconv3x3's
dispatch and upd_geometry_ok: the v4 condition, the unit-route condition, UPD_* / UP_MAX_R, the window and run
rules in fp32, the R loop), not evidence about the device: every case asserts the route it is listed under, so a
later change to the dispatch fails here loudly instead of silently emptying a route's case list
(``test_every_route_has_cases``, no GPU). The host evaluates bilin_src without FP contraction and the device may
contract ``scale * (dst + 0.5) - 0.5`` into one fma; ``test_dma_geometry_table`` asserts that both forms pick the
same source rows and columns at every DMA shape listed here. Behaviour separates the unit route from the general
one (``test_unit_vs_general_nonfinite_neighbour``): a NaN in z one column outside a tap's support is NaN on the
general form (it adds 0 * the next column) and finite on the unit form; asserted once in each direction. No
other confirmation of the route list was made (no kernel trace).

Branch -> case map
  unit kernel <1..4>: W in {1, 63, 64, 65, 130, 192, 257, 300} (strip edges on both sides, 3 strips, 5 strips =
      ngroups 2 with three idle waves that still reach amax_commit) x H in {1, 2, 31, 32, 33, 64, 65} (chunk edges;
      at 64 the last row of a chunk has oy1 == H), every pair once, CO / activation / z pitch / y layout (dense,
      NHWC4 slice, NCHW) cycling: test_unit_every_strip_and_chunk_edge. CO x every activation:
      test_unit_every_co_and_activation. scale / bias / slope absent: test_unit_absent_operands. y_amax at N = 3:
      test_unit_y_amax. Data x 50, x 1e-3: test_unit_data_scale. Negations (ac = False, z.sw = 40 at Co = 4,
      Co = 5): test_unit_negations_keep_the_bits.
  DMA kernel <ACT, PL>: Ho = 5 Hi and Wo < 32 (2, 2, 10, 5); ragged last tile with 1 and 8 live columns, three
      waves not wlive -> vmcnt(0) branch (4, 4, 20, 33 / 40); middle intervals of exactly 5 rows, Ho = 255 and
      256 = UP_MAX_R with ty0 / thi full (51, 3, 255 / 256, 9); window of exactly UPD_NSC (3, 8, 16, 33); both
      align_corners modes, PL both, N in {1, 3}, z dense / padded, y dense / inner / concat (fp32), dense / pad8 /
      concat (planes): test_dma_row_and_window_geometry. Leaves the route and keeps the bits: (52, 3, 260, 9),
      (3, 9, 16, 33), (6, 20, 30, 100): test_dma_geometry_leaves_route. Model shapes 20 -> 160 and 20 -> 256 x 192
      at Co 32: test_dma_model_shapes. Co in {32, 64, 96} x N in {1, 3}: test_dma_channel_blocks_and_frames.
      Every ACT instantiation and relu / sigmoid through -1, PL both: test_dma_every_activation. y_amax, also on
      the ragged tile: test_dma_y_amax. Data scale: test_dma_data_scale. Refusals into the fused kernel with the
      same bits (y.sc != 1, Co = 48, z base 4-byte aligned): test_dma_refusals_keep_the_bits.
  fused kernel <4, ACT>: every ACT and -1: test_fused_v4_every_activation; NCHW y at Co = 8 (scalar-store tail):
      test_fused_v4_nchw_tail; planes at Co = 24: test_fused_v4_planes; y_amax with per_row % 256 != 0 (lanes past
      the row stay for amax_commit): test_fused_y_amax. <1, -1>: Co in {1, 5, 17}, odd y, z as an NCHW view:
      test_fused_v1. Geometry, both modes: downsampling (9, 7, 4, 3), (20, 20, 7, 5) (y0 != cur + 1: full rebuild),
      identity at Co = 8, Hi / Wi / Ho / Wo = 1 singly and together, (7, 9, 20, 13), (11, 4, 61, 8), Ho = 260:
      test_fused_geometry. Row ranges: every unit-test shape shrinks R to 4; R = 8 with three row blocks
      (N 11, Co 1, (3, 16, 17, 65536): chunks 256, 12.3 M outputs) and R = 16 with three row blocks (N 11, Co 1,
      (3, 16, 33, 65536), 23.8 M outputs): test_fused_long_row_ranges, R asserted through route_of. R >= 32 with
      more than one row block needs > 100 MB of output: left to the benchmark's workload. Data scale:
      test_fused_data_scale.
  separable: VW 4 and 1 at three shapes, dense, inner and NCHW y: test_separable_against_fp64; data scale:
      test_separable_data_scale; y_amax -> PrpeError: test_separable_refuses_y_amax.
  host: workspace one byte short or 4 bytes off 16 falls through to the one-pass route, same bits, workspace
      never written: test_workspace_fall_through; EINVAL with untouched buffers (z.n != y.n, z.c != 9 y.c, PReLU
      without slope, planes with Co % 8, misaligned y, strided y, a workspace): test_einval_leaves_buffers.
      tests/test_abi_and_host.py asserts none of these, so none is skipped.

Single-line mutations each group catches (by reading, not by running)
  dx and dy swapped in the tap index: every fp64 comparison (z is random per tap); pinned for the reference itself
      by test_reference_hand_case.
  xs_lo off by one (DMA window): the first / last window column is wrong or NaN -> value check of every DMA case
      with ox0 > 0 (Wo 33, 40, 160, 192) and of Wi = 2 / 3 (the window is the whole row).
  zbytes one pixel short: the last pixel of z reads as zero through the descriptor -> value check at the last
      output rows / columns of every DMA case, dense and padded z.
  vmcnt(4) on the planes path (8 stores per row there): rows read before their DMA landed -> the PL cases at the
      minimum ratio (2, 2, 10, 5), (4, 4, 20, *), (51, 3, 255 / 256, 9), bit equality and fp64.
  live dropped from the DMA store: columns >= Wo written -> Guarded.untouched at Wo 5, 9, 33, 40 (dense y: the
      next row's pixels change -> value check).
  r1 off by one in the unit kernel: the last row of a chunk lacks its dy = 2 term, or reads row H -> value / NaN
      at H 31, 32, 33, 64, 65.
  jv ignoring px < W: the strip's right halo reads the next row's first pixel (dense z) or the NaN pitch ->
      value / NaN at W 63, 64, 65, 130, 257, 300.
  par not flipped: A / B swapped after the first source interval -> value check of every DMA case with Hi > 2.

Measured on the MI355X, largest err / allowance per route (``held`` runs once per fp32 launch): unit 0.251,
DMA 0.297, fused <4> 0.303, fused <1> 0.332, separable 0.297. No ratio came out above 1 and no kernel or host rule
needed a change. 342 GPU cases and 4 host cases, 8 s; the two long-row-range cases take 1.1 s and 1.9 s (12.3 M and
23.8 M outputs, references included), every other case under 0.2 s.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from prpe import ops
from prpe._lib import ACT, PrpeError, lib
from test_gpu_ops import _decode_planes, _g, act_ref, rnd
from test_gpu_rowops import DEV, SENT, Guarded, dev_in, g_nhwc, in_nhwc, nhwc_layout, same_bits, scaled_tol  # noqa: F401

gpu = pytest.mark.gpu
ACTS = ["none", "relu", "silu", "prelu", "gelu", "sigmoid"]
BIG = float(torch.tensor(3.0e38))
RATIO = {}                 # largest err / allowance per route, printed when the module ends
COUNT = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    if RATIO:
        print("\nlargest err / allowance per route: " +
              ", ".join(f"{k} {v:.3f} ({COUNT[k]} checks)" for k, v in sorted(RATIO.items())))


# ====================================================================== the reference
def upconv_ref(z, Ho, Wo, ac, scale, bias, slope, act, dtype, with_pre=False):
    """Stage 2 on z [N, 9 Co, Hi, Wi] (CPU): bilinear resize of every tap map to (Ho, Wo), then
    pre[n, c, oy, ox] = sum_{dy, dx} U[n, (3 dy + dx) Co + c, oy + dy - 1, ox + dx - 1] (zero outside the output
    grid), scale, bias, activation; in ``dtype``. Frame by frame (memory), never pixel by pixel."""
    Co = z.shape[1] // 9
    outs, pres = [], []
    for n in range(z.shape[0]):
        U = F.interpolate(z[n:n + 1].to(dtype), (Ho, Wo), mode="bilinear", align_corners=ac)
        P = F.pad(U, (1, 1, 1, 1))
        pre = torch.zeros(1, Co, Ho, Wo, dtype=dtype)
        for dy in range(3):
            for dx in range(3):
                t = 3 * dy + dx
                pre = pre + P[:, t * Co:(t + 1) * Co, dy:dy + Ho, dx:dx + Wo]
        if scale is not None:
            pre = pre * scale.to(dtype).view(1, -1, 1, 1)
        if bias is not None:
            pre = pre + bias.to(dtype).view(1, -1, 1, 1)
        outs.append(act_ref(pre, act, slope.to(dtype) if slope is not None else None))
        pres.append(pre)
    out = torch.cat(outs)
    return (out, torch.cat(pres)) if with_pre else out


@pytest.mark.parametrize("ac", [True, False])
def test_reference_hand_case(ac):
    """2 x 2 -> 3 x 3, Co = 2. A 2 x 2 map [[a, b], [c, d]] resized to 3 x 3 is
    [[a, (a+b)/2, b], [(a+c)/2, (a+b+c+d)/4, (b+d)/2], [c, (c+d)/2, d]] in both modes (align_corners=False puts the
    sources at 0, 0.5 and 7/6, and 7/6 clamps to the last sample). Two taps are non-zero:
      tap (dy 0, dx 2), channel 1 = z channel (3*0 + 2)*2 + 1 = 5, map [[1, 2], [3, 4]]:
          U = [[1, 1.5, 2], [2, 2.5, 3], [3, 3.5, 4]], pre[1][oy][ox] = U[oy - 1][ox + 1]
      tap (dy 2, dx 0), channel 0 = z channel (3*2 + 0)*2 + 0 = 12, map [[10, 20], [30, 40]]:
          U = [[10, 15, 20], [20, 25, 30], [30, 35, 40]], pre[0][oy][ox] = U[oy + 1][ox - 1]
    then out[0] = 2 pre[0] + 1 and out[1] = pre[1] + 0.5."""
    z = torch.zeros(1, 18, 2, 2)
    z[0, 5] = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    z[0, 12] = torch.tensor([[10.0, 20.0], [30.0, 40.0]])
    want = torch.tensor([[[[1.0, 41.0, 51.0], [1.0, 61.0, 71.0], [1.0, 1.0, 1.0]],
                          [[0.5, 0.5, 0.5], [2.0, 2.5, 0.5], [3.0, 3.5, 0.5]]]], dtype=torch.float64)
    for dtype in (torch.float64, torch.float32):
        got = upconv_ref(z, 3, 3, ac, torch.tensor([2.0, 1.0]), torch.tensor([1.0, 0.5]), None, "none", dtype)
        torch.testing.assert_close(got.double(), want, rtol=0, atol=1e-6 if dtype == torch.float32 else 1e-14)
    # swapped dy / dx would read z channel 12 as tap (0, 2): not this result
    relu = upconv_ref(z, 3, 3, ac, torch.tensor([-2.0, 1.0]), None, None, "relu", torch.float64)
    assert float(relu[0, 0].abs().max()) == 0.0 and abs(float(relu[0, 1, 2, 1]) - 3.0) < 1e-12


# ====================================================================== host dispatch, restated
f32 = np.float32
UPD_W, UPD_C, UPD_NSC, UP_MAX_R, UPU_R = 32, 32, 8, 256, 32


def bilin_i0(dst, n_in, n_out, ac, fused=False):
    """(i0, i1) of bilin_src / bilin_src_h in fp32. fused: scale * (dst + 0.5) - 0.5 as one fma (the product
    of two floats is exact in double; the one rounding to float follows)."""
    if ac:
        scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        src = scale * f32(dst)
    else:
        scale = f32(n_in) / f32(n_out)
        if fused:
            src = f32(float(scale) * (float(dst) + 0.5) - 0.5)
        else:
            src = scale * (f32(dst) + f32(0.5)) - f32(0.5)
        if src < 0:
            src = f32(0)
    i0 = min(int(src), n_in - 1)
    return i0, (i0 + 1 if i0 < n_in - 1 else i0)


def upd_geometry_ok(Hi, Wi, Ho, Wo, ac, zsh, zsw, zc, fused=False):
    if Hi < 2 or Ho < 5 * Hi:
        return False
    for ox0 in range(0, Wo, UPD_W):
        lo = bilin_i0(ox0 - 1 if ox0 > 0 else 0, Wi, Wo, ac, fused)[0]
        hi = bilin_i0(ox0 + UPD_W if ox0 + UPD_W < Wo else Wo - 1, Wi, Wo, ac, fused)[1]
        if hi - lo + 1 > UPD_NSC:
            return False
    prev, run, first = -1, 0, True
    for oy in range(Ho):
        y0 = bilin_i0(oy, Hi, Ho, ac, fused)[0]
        if y0 != prev:
            if prev >= 0 and not first and run < 5:
                return False
            if prev >= 0:
                first = False
            prev, run = y0, 0
        run += 1
    return ((Hi - 1) * zsh + (Wi - 1) * zsw + zc) * 4 < 2 ** 31


def route_shape(zshape, zstride, zalign, yshape, ystride, yalign, ac, planes=False, separable=False):
    """The kernel prpe_upconv3x3 launches for these views: ("sep", VW), ("unit", Co), ("dma",) or
    ("fused", VW, R). zalign / yalign: base address % 16 (% 32 is the planes refusal, not a route)."""
    N, Ho, Wo, Co = yshape
    _, Hi, Wi, zc = zshape
    zsn, zsh, zsw, zsc = zstride
    ysn, ysh, ysw, ysc = ystride
    v4 = (Co % 4 == 0 and zsc == 1 and zsw % 4 == 0 and zsh % 4 == 0 and zsn % 4 == 0 and zalign == 0 and
          (ysc != 1 or (ysw % 4 == 0 and ysh % 4 == 0 and ysn % 4 == 0 and yalign == 0)))
    vw = 4 if v4 else 1
    if separable:
        return ("sep", vw)
    if ac and Co <= 4 and (Hi, Wi) == (Ho, Wo) and not planes and zsc == 1 and zsw == zc:
        return ("unit", Co)
    if v4 and Co % UPD_C == 0 and ysc == 1 and zsc == 1 and Ho <= UP_MAX_R and \
            upd_geometry_ok(Hi, Wi, Ho, Wo, ac, zsh, zsw, zc):
        return ("dma",)
    chunks = (Wo * (Co // vw) + 255) // 256
    R = min(UP_MAX_R, 256)
    while R > 4 and N * ((Ho + R - 1) // R) * chunks < 8192:
        R //= 2
    return ("fused", vw, R)


def route_of(z, y, ac, planes=False, separable=False):
    return route_shape(tuple(z.shape), z.stride(), z.data_ptr() % 16, tuple(y.shape), y.stride(), y.data_ptr() % 16,
                       ac, planes, separable)


# ====================================================================== cases
def mk(z, Ho, Wo, ac, act, sc, bi, sl, zscale=1.0):
    """z: CPU logical NHWC [N, Hi, Wi, 9 Co]. Operands and both references, computed once, never modified."""
    N, Hi, Wi, zc = z.shape
    c = SimpleNamespace(z=z, N=N, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, Co=zc // 9, ac=ac, act=act, sc=sc, bi=bi,
                        sl=sl if act == "prelu" else None, zscale=zscale, cache={})
    zn = z.permute(0, 3, 1, 2)
    r64, p64 = upconv_ref(zn, Ho, Wo, ac, sc, bi, c.sl, act, torch.float64, with_pre=True)
    r32 = upconv_ref(zn, Ho, Wo, ac, sc, bi, c.sl, act, torch.float32)
    c.ref = r64.permute(0, 2, 3, 1).contiguous()         # NHWC, fp64
    c.pre = p64.permute(0, 2, 3, 1).contiguous()
    c.e_ref = float((r32.double() - r64).abs().max())
    c.nout = c.ref.numel()
    c.unit_geom = ac and (Hi, Wi) == (Ho, Wo)
    c.has = (sc is not None, bi is not None)
    return c


@functools.lru_cache(maxsize=None)
def case(N, Hi, Wi, Ho, Wo, Co, ac, act="gelu", zscale=1.0, has=(True, True), seed=0):
    sd = 9000 + 7 * Hi + 11 * Wi + 13 * Ho + 17 * Wo + 19 * Co + 23 * N + seed
    z = rnd(N, Hi, Wi, 9 * Co, seed=sd, scale=zscale)
    sc = torch.rand(Co, generator=_g(sd + 1)) + 0.5 if has[0] else None
    bi = rnd(Co, seed=sd + 2, scale=zscale) if has[1] else None
    sl = torch.rand(Co, generator=_g(sd + 3)) * 0.4
    return mk(z, Ho, Wo, ac, act, sc, bi, sl, zscale)


def YARD_UNIT(act, zscale, has):
    return case(2, 33, 65, 33, 65, 3, True, act, zscale, has)


def YARD_GEN(act, zscale, has):
    return case(2, 7, 9, 20, 13, 24, False, act, zscale, has)


def allowance(c):
    """Elementwise allowance of a case (see the module docstring)."""
    e = c.e_ref if c.nout >= 4096 else (YARD_UNIT if c.unit_geom else YARD_GEN)(c.act, c.zscale, c.has).e_ref
    a = torch.full_like(c.ref, 4.0 * e)
    if c.act in ("silu", "sigmoid", "gelu"):
        a = a + 4 * torch.finfo(torch.float32).eps * c.ref.float().double().abs() + 1e-35
    if c.act == "gelu":
        a = a + 2.0 ** -22 * c.pre.abs()
    return a


def held(fam, what, c, got):
    """got (CPU NHWC fp32) against the fp64 reference within the case's allowance; prints the ratio."""
    assert got.shape == c.ref.shape
    assert not got.isnan().any(), f"{what}: NaN in the output (a read outside z)"
    err = (got.double() - c.ref).abs()
    a = allowance(c)
    r = float(torch.where(err == 0, torch.zeros_like(err), err / a).max())
    RATIO[fam] = max(RATIO.get(fam, 0.0), r)
    COUNT[fam] = COUNT.get(fam, 0) + 1
    print(f"\n[{fam}] {what}: err {float(err.max()):.3e} e_ref {c.e_ref:.3e} ({c.nout} outputs) ratio {r:.3f}")
    assert r <= 1.0, (what, r)


def fam_of(route):
    return {"sep": "separable", "unit": "unit", "dma": "dma"}.get(route[0]) or f"fused{route[1]}"


def z_layout(c, kind):
    n, h, w, ch = c.z.shape
    if kind == "pitch":                                   # unit route: pixel pitch 9 Co, padded rows and frames
        sh = (w + 3) * ch
        return (sh * (h + 2), sh, ch, 1), sh + ch
    if kind == "mis4":                                    # dense, base one float off the 16-byte grid
        return (h * w * ch, w * ch, ch, 1), 1
    if kind == "sw40":                                    # Co = 4: pixel pitch 40 instead of 36
        return (h * w * 40, w * 40, 40, 1), 0
    return nhwc_layout(n, h, w, ch, kind)


def z_dev(c, kind):
    st, sf = z_layout(c, kind)
    return dev_in(c.z, st, sf)


class Out:
    """y as a Guarded view in one of the layouts; ``.view`` is the logical NHWC tensor handed to the library."""

    def __init__(self, n, h, w, co, kind):
        self.kind = kind
        if kind == "nchw":                                # an NCHW tensor seen through ops.nhwc
            self.g = Guarded((n, co, h, w))
            self.view = ops.nhwc(self.g.view)
            return
        if kind == "nhwc4":                               # channels [0, co) of a 4-channel pixel
            st, sf = (h * w * 4, w * 4, 4, 1), 0
        elif kind == "pad8":                              # pixels, rows and frames padded by multiples of 8
            sw = co + 8
            sh = (w + 1) * sw
            st, sf = ((h + 2) * sh, sh, sw, 1), sh + sw + 8
        else:
            st, sf = nhwc_layout(n, h, w, co, kind)
        self.g = Guarded((n, h, w, co), st, sf)
        self.view = self.g.view

    def cpu(self):
        t = self.g.cpu()
        return (t.permute(0, 2, 3, 1) if self.kind == "nchw" else t).contiguous()

    def untouched(self):
        return self.g.untouched()


def dptr(t):
    return None if t is None else t.to(DEV)


def launch(c, z, y, *, planes=False, separable=False, ya=None):
    ops.upconv3x3(z, y, c.ac, dptr(c.sc), dptr(c.bi), dptr(c.sl), c.act, separable=separable, y_planes=planes,
                  y_amax=ya)
    torch.cuda.synchronize()


def sep_bits(c):
    """The separable result of the case's operands (dense z and y), once per case."""
    if "sep" not in c.cache:
        y = Out(c.N, c.Ho, c.Wo, c.Co, "dense")
        launch(c, z_dev(c, "dense"), y.view, separable=True)
        c.cache["sep"] = y.cpu()
    return c.cache["sep"]


def fused_bits(c):
    """A DMA case's operands through the fused kernel <4> (an NCHW y keeps v4 and is refused by the DMA route),
    once per case."""
    if "fused" not in c.cache:
        z = z_dev(c, "dense")
        y = Out(c.N, c.Ho, c.Wo, c.Co, "nchw")
        assert route_of(z, y.view, c.ac)[:2] == ("fused", 4)
        launch(c, z, y.view)
        c.cache["fused"] = y.cpu()
    return c.cache["fused"]


def run(c, expect, *, zk="dense", yk="dense", planes=False, amax=False, separable=False, what=""):
    """One launch in the harness: the route restated and asserted, value against fp64, bits against the
    separable form, nothing written outside y. Planes: the fp32 result of the same route first."""
    z = z_dev(c, zk)
    y = Out(c.N, c.Ho, c.Wo, c.Co, yk)
    r = route_of(z, y.view, c.ac, False, separable)
    assert r[:len(expect)] == expect, (r, expect)
    slots, keep = None, int(c.N > 1)                      # keep: the last frame's slot already holds more
    if amax:
        slots = torch.tensor([SENT] + [0.0] * (c.N - keep) + [BIG] * keep + [SENT], device=DEV)
    launch(c, z, y.view, separable=separable, ya=slots[1:c.N + 1] if amax else None)
    got = y.cpu()
    tag = f"{what} {c.N}x{c.Hi}x{c.Wi}->{c.Ho}x{c.Wo} Co{c.Co} ac{int(c.ac)} {c.act} z:{zk} y:{yk}"
    held(fam_of(r), tag, c, got)
    assert y.untouched(), tag
    assert same_bits(got, sep_bits(c)), tag
    want = got.abs().amax(dim=(1, 2, 3))
    if amax:
        s = slots.cpu()
        assert s[0] == SENT and s[-1] == SENT
        assert torch.equal(s[1:c.N + 1 - keep], want[:c.N - keep]) and (not keep or float(s[c.N]) == BIG), (s, want)
    if planes:
        assert route_of(z, y.view, c.ac, True)[:len(expect)] == expect
        yp = Out(c.N, c.Ho, c.Wo, c.Co, yk)
        ya = torch.zeros(c.N, device=DEV) if amax else None
        launch(c, z, yp.view, planes=True, ya=ya)
        assert ya is None or torch.equal(ya.cpu(), want), tag
        hi, lo = _decode_planes(yp.cpu())
        assert torch.equal(hi, got.to(torch.bfloat16).float()), tag
        assert torch.equal(lo, (got - hi).to(torch.bfloat16).float()), tag
        assert yp.untouched(), tag
    return got


# ---------------------------------------------------------------------- the case lists (shared with the no-GPU checks)
UNIT_W = [1, 63, 64, 65, 130, 192, 257, 300]
UNIT_H = [1, 2, 31, 32, 33, 64, 65]
UNIT_GRID = [(w, h, (i * len(UNIT_H) + j) % 4 + 1, ACTS[(i + 2 * j) % 6], ("dense", "pitch")[(i + j) % 2],
              ("dense", "nhwc4", "nchw")[(i + j // 2) % 3])
             for i, w in enumerate(UNIT_W) for j, h in enumerate(UNIT_H)]

DMA_STAY = [(2, 2, 10, 5), (4, 4, 20, 33), (4, 4, 20, 40), (51, 3, 255, 9), (51, 3, 256, 9), (3, 8, 16, 33)]
DMA_LEAVE = [(52, 3, 260, 9), (3, 9, 16, 33), (6, 20, 30, 100)]
DMA_MODEL = [(20, 20, 160, 160), (20, 20, 256, 192)]

FUSED_GEOM = [(9, 7, 4, 3), (20, 20, 7, 5), (6, 5, 6, 5), (1, 5, 7, 9), (5, 1, 9, 7), (5, 4, 1, 9), (4, 5, 9, 1),
              (1, 1, 1, 1), (1, 1, 6, 7), (5, 6, 1, 1), (7, 9, 20, 13), (11, 4, 61, 8), (13, 3, 260, 5)]
LONG_R = [(8, 11, 3, 16, 17, 65536), (16, 11, 3, 16, 33, 65536)]


def dense(n, h, w, c):
    return (h * w * c, w * c, c, 1)


def test_dma_geometry_table():
    """The restated host rule keeps / refuses the listed DMA shapes in both align_corners modes, and the
    uncontracted (host) and contracted (device) forms of bilin_src pick the same source rows and columns there."""
    for ac in (True, False):
        for shp in DMA_STAY + DMA_MODEL + DMA_LEAVE:
            Hi, Wi, Ho, Wo = shp
            ok = Ho <= UP_MAX_R and upd_geometry_ok(Hi, Wi, Ho, Wo, ac, Wi * 288, 288, 288)
            assert ok == (shp not in DMA_LEAVE), (shp, ac)
            for n_in, n_out in ((Hi, Ho), (Wi, Wo)):
                for d in range(n_out):
                    assert bilin_i0(d, n_in, n_out, ac) == bilin_i0(d, n_in, n_out, ac, fused=True), (shp, ac, d)
    # the window of (3, 8, 16, 33) is exactly UPD_NSC wide, that of (3, 9, 16, 33) one more
    assert bilin_i0(32, 8, 33, True)[1] - bilin_i0(0, 8, 33, True)[0] + 1 == UPD_NSC
    assert bilin_i0(32, 9, 33, True)[1] - bilin_i0(0, 9, 33, True)[0] + 1 == UPD_NSC + 1
    # (51, 3, 255, 9): every middle interval has exactly 5 rows
    rows = [bilin_i0(d, 51, 255, False)[0] for d in range(255)]
    assert {rows.count(k) for k in range(1, 50)} == {5}


def test_every_route_has_cases():
    """Each route's case list is non-empty according to the restated dispatch (dense, aligned views)."""
    def r(N, Hi, Wi, Ho, Wo, Co, ac, **kw):
        return route_shape((N, Hi, Wi, 9 * Co), dense(N, Hi, Wi, 9 * Co), 0, (N, Ho, Wo, Co), dense(N, Ho, Wo, Co), 0,
                           ac, **kw)
    assert all(r(2, h, w, h, w, co, True) == ("unit", co) for w, h, co, *_ in UNIT_GRID) and len(UNIT_GRID) == 56
    assert {co for _, _, co, *_ in UNIT_GRID} == {1, 2, 3, 4}
    for ac in (True, False):
        assert all(r(1, *s, 32, ac) == ("dma",) for s in DMA_STAY + DMA_MODEL)
        assert all(r(1, *s, 32, ac)[:2] == ("fused", 4) for s in DMA_LEAVE)
        assert all(r(2, *s, 8, ac)[:2] == ("fused", 4) or (ac and s[:2] == s[2:]) for s in FUSED_GEOM)
        assert all(r(2, *s, 5, ac) == ("fused", 1, 4) for s in FUSED_GEOM)
    assert r(2, 6, 5, 6, 5, 8, True) == ("fused", 4, 4) and r(2, 6, 5, 6, 5, 4, True) == ("unit", 4)
    for R, N, Hi, Wi, Ho, Wo in LONG_R:
        assert r(N, Hi, Wi, Ho, Wo, 1, True) == ("fused", 1, R) and (Ho + R - 1) // R == 3
    assert r(2, 7, 9, 20, 13, 24, False, separable=True) == ("sep", 4)
    assert r(2, 7, 9, 20, 13, 5, False, separable=True) == ("sep", 1)


# ====================================================================== unit kernel
@gpu
@pytest.mark.parametrize("W,H,co,act,zk,yk", UNIT_GRID)
def test_unit_every_strip_and_chunk_edge(W, H, co, act, zk, yk):
    run(case(2, H, W, H, W, co, True, act), ("unit", co), zk=zk, yk=yk)


@gpu
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("co", [1, 2, 3, 4])
def test_unit_every_co_and_activation(co, act):
    run(case(2, 33, 130, 33, 130, co, True, act, seed=1), ("unit", co), zk="pitch", yk=("dense", "nhwc4")[co & 1])


@gpu
@pytest.mark.parametrize("has", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("co", [1, 2, 3, 4])
def test_unit_absent_operands(co, has):
    """scale, bias and (every activation but PReLU) slope absent."""
    run(case(2, 33, 65, 33, 65, co, True, "silu", has=has), ("unit", co), zk="pitch")


@gpu
@pytest.mark.parametrize("W,H", [(300, 65), (130, 33), (64, 64), (1, 1)])
@pytest.mark.parametrize("co", [1, 2, 3, 4])
def test_unit_y_amax(co, W, H):
    """N = 3; at W = 300 the second strip group has three idle waves that still reach amax_commit."""
    run(case(3, H, W, H, W, co, True, "prelu" if co & 1 else "gelu"), ("unit", co), amax=True,
        yk=("dense", "nhwc4", "nchw")[co % 3])


@gpu
@pytest.mark.parametrize("zscale", [50.0, 1e-3])
def test_unit_data_scale(zscale):
    run(case(2, 33, 130, 33, 130, 3, True, "gelu", zscale), ("unit", 3))
    run(case(2, 33, 130, 33, 130, 4, True, "silu", zscale), ("unit", 4), zk="pitch")


def narrow(c, co):
    """The case of the first ``co`` output channels of ``c`` (its taps' first co channels, same scale / bias /
    slope): the widened case's y[..., :co] is this case's y."""
    z = c.z.view(c.N, c.Hi, c.Wi, 9, c.Co)[..., :co].reshape(c.N, c.Hi, c.Wi, 9 * co).contiguous()
    return mk(z, c.Ho, c.Wo, c.ac, c.act, c.sc[:co].clone(), c.bi[:co].clone(),
              c.sl[:co].clone() if c.sl is not None else None)


@gpu
@pytest.mark.parametrize("act", ["gelu", "prelu"])
def test_unit_negations_keep_the_bits(act):
    """Each unit-route condition flipped once: the general kernels give the unit kernel's bits on finite z."""
    H, W = 33, 130
    c4 = case(2, H, W, H, W, 4, True, act, seed=2)
    unit = run(c4, ("unit", 4))
    # align_corners = False on the same grid: src = (dst + 0.5) - 0.5 = dst exactly, every weight 0
    cf = mk(c4.z, H, W, False, act, c4.sc, c4.bi, c4.sl)
    assert same_bits(run(cf, ("fused", 4)), unit)
    # z.sw = 40 at Co = 4
    assert same_bits(run(c4, ("fused", 4), zk="sw40"), unit)
    # Co = 5: its first four channels are a Co = 4 case
    c5 = case(2, H, W, H, W, 5, True, act, seed=2)
    n4 = narrow(c5, 4)
    got5 = run(c5, ("fused", 1))
    assert same_bits(got5[..., :4].contiguous(), run(n4, ("unit", 4)))


@gpu
def test_unit_vs_general_nonfinite_neighbour():
    """A NaN at z[n, r, xc] in tap (dy, dx), channel ch: the tap sum of output (r + 1 - dy, xc + 1 - dx) alone
    contains it. The unit kernel makes exactly that output NaN. The general form also evaluates
    (1 - 0) z[x0] + 0 * z[x0 + 1] (and the same down the rows), so its outputs one column to the left and one
    row up are NaN too. This is how the two routes differ in behaviour, in both directions."""
    H, W, co = 9, 70, 3
    c = case(1, H, W, H, W, co, True, "none", seed=3)
    r, xc, dy, dx, ch = 4, 65, 1, 2, 1
    z = c.z.clone()
    z[0, r, xc, (3 * dy + dx) * co + ch] = float("nan")
    oy, ox = r + 1 - dy, xc + 1 - dx
    outs = {}
    for name, ac in (("unit", True), ("general", False)):
        zd = dev_in(z, dense(1, H, W, 9 * co))
        y = Out(1, H, W, co, "dense")
        assert route_of(zd, y.view, ac)[0] == ("unit" if ac else "fused")
        ops.upconv3x3(zd, y.view, ac, dptr(c.sc), dptr(c.bi), None, "none")
        torch.cuda.synchronize()
        assert y.untouched()
        outs[name] = y.cpu()
    nan_u = outs["unit"].isnan().nonzero().tolist()
    nan_g = outs["general"].isnan().nonzero().tolist()
    assert nan_u == [[0, oy, ox, ch]]
    assert sorted(nan_g) == sorted([[0, oy, ox, ch], [0, oy, ox - 1, ch], [0, oy - 1, ox, ch], [0, oy - 1, ox - 1, ch]])
    fin = ~outs["general"].isnan()
    assert torch.equal(outs["unit"][fin], outs["general"][fin])
    assert float((outs["unit"][fin].double() - c.ref[fin]).abs().max()) <= 4 * YARD_UNIT("none", 1.0, (True, True)).e_ref


# ====================================================================== DMA kernel
DMA_Y32 = ["dense", "inner", "concat"]
DMA_YPL = ["dense", "pad8", "concat"]


@gpu
@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("shp", DMA_STAY)
def test_dma_row_and_window_geometry(shp, ac, planes):
    i = DMA_STAY.index(shp) + int(ac)
    N = (3, 1)[i % 2] if shp != (2, 2, 10, 5) else 3
    c = case(N, *shp, 32, ac, ACTS[(i + 3 * planes) % 6])
    run(c, ("dma",), zk=("inner", "dense")[(i + planes) % 2], yk=(DMA_YPL if planes else DMA_Y32)[i % 3],
        planes=planes)
    assert same_bits(fused_bits(c), sep_bits(c))


@gpu
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("shp", DMA_LEAVE)
def test_dma_geometry_leaves_route(shp, ac):
    """Ho > UP_MAX_R, a source window of UPD_NSC + 1 columns: the fused kernel, the same bits."""
    planes = shp[3] != 100
    run(case(1, *shp, 32, ac, "silu"), ("fused", 4), zk="inner", yk="pad8" if planes else "inner", planes=planes)


@gpu
@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("shp", DMA_MODEL)
def test_dma_model_shapes(shp, planes):
    c = case(1, *shp, 32, True, "gelu" if shp[2] == 256 else "silu")
    run(c, ("dma",), zk="dense", yk="dense", planes=planes, amax=not planes)


@gpu
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("co", [32, 64, 96])
def test_dma_channel_blocks_and_frames(co, N):
    c = case(N, 4, 4, 20, 40, co, co != 64, "prelu")
    run(c, ("dma",), zk=("dense", "inner")[N // 2], yk=DMA_YPL[(co // 32) % 3], planes=True, amax=True)
    assert same_bits(fused_bits(c), sep_bits(c))


@gpu
@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("act", ACTS)
def test_dma_every_activation(act, planes):
    """ACT = none, silu, prelu, gelu as compile-time constants; relu and sigmoid through the -1 instantiation."""
    run(case(2, 4, 5, 23, 37, 32, False, act, seed=4), ("dma",), zk="inner", yk="pad8" if planes else "inner",
        planes=planes)


@gpu
@pytest.mark.parametrize("shp", [(4, 4, 20, 33), (4, 4, 20, 40), (2, 2, 10, 5), (3, 8, 16, 33)])
def test_dma_y_amax(shp):
    """The ragged tile's dead lanes and the three waves without a live column contribute 0."""
    run(case(3, *shp, 64, True, "none", seed=5), ("dma",), zk="inner", yk="concat", amax=True)
    run(case(3, *shp, 32, False, "silu", seed=5), ("dma",), amax=True)


@gpu
@pytest.mark.parametrize("zscale", [50.0, 1e-3])
def test_dma_data_scale(zscale):
    run(case(2, 4, 5, 23, 37, 32, False, "gelu", zscale), ("dma",), planes=True)
    run(case(2, 4, 5, 23, 37, 32, True, "silu", zscale), ("dma",), zk="inner", yk="inner")


@gpu
@pytest.mark.parametrize("ac", [True, False])
def test_dma_refusals_keep_the_bits(ac):
    c = case(2, 4, 4, 20, 40, 32, ac, "gelu", seed=6)
    dma = run(c, ("dma",))
    # y.sc != 1
    assert same_bits(run(c, ("fused", 4), yk="nchw"), dma)
    # a z base address that is only 4-byte aligned
    assert same_bits(run(c, ("fused", 1), zk="mis4"), dma)
    # an unaligned y
    assert same_bits(run(c, ("fused", 1), yk="odd"), dma)
    # Co = 48: its first 32 channels are a Co = 32 case
    c48 = case(2, 4, 4, 20, 40, 48, ac, "gelu", seed=6)
    got = run(c48, ("fused", 4), planes=True)
    assert same_bits(got[..., :32].contiguous(), run(narrow(c48, 32), ("dma",)))


# ====================================================================== fused kernel
@gpu
@pytest.mark.parametrize("yk", ["dense", "inner", "concat"])
@pytest.mark.parametrize("act", ACTS)
def test_fused_v4_every_activation(act, yk):
    run(case(2, 7, 9, 20, 13, 24, False, act), ("fused", 4, 4), zk=("dense", "inner", "concat")[ACTS.index(act) % 3],
        yk=yk)


@gpu
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("shp", [(7, 9, 20, 13), (6, 5, 6, 5), (4, 4, 20, 40)])
def test_fused_v4_nchw_tail(shp, ac):
    """Co % 4 == 0 with y.sc != 1: VW = 4 and the scalar stores after the two vector branches."""
    run(case(2, *shp, 8, ac, "silu"), ("fused", 4), zk="inner", yk="nchw")


@gpu
@pytest.mark.parametrize("yk", ["dense", "pad8", "concat"])
@pytest.mark.parametrize("shp,ac", [((7, 9, 20, 13), False), ((11, 4, 61, 8), True), ((9, 7, 4, 3), False)])
def test_fused_v4_planes(shp, ac, yk):
    """Co % 8 == 0 but not % 32: the planes store of the fused kernel."""
    run(case(2, *shp, 24, ac, "gelu"), ("fused", 4), zk="inner", yk=yk, planes=True)


@gpu
@pytest.mark.parametrize("N,shp,co,yk", [(3, (7, 9, 20, 13), 8, "dense"), (3, (6, 20, 30, 100), 24, "inner"),
                                          (2, (7, 9, 20, 13), 5, "odd"), (3, (4, 4, 20, 40), 17, "nchw"),
                                          (3, (1, 1, 1, 1), 8, "dense")])
def test_fused_y_amax(N, shp, co, yk):
    """per_row = 26, 600 (three chunks, the last with 168 idle lanes), 65, 680, 2: never a multiple of 256."""
    run(case(N, *shp, co, False, "prelu" if co != 5 else "none"), ("fused",), yk=yk, amax=True)


@gpu
@pytest.mark.parametrize("zk,yk", [("dense", "dense"), ("odd", "odd"), ("nchw", "dense"), ("inner", "odd"),
                                   ("nchw", "nchw"), ("concat", "inner")])
@pytest.mark.parametrize("co", [1, 5, 17])
def test_fused_v1(co, zk, yk):
    """VW = 1: Co % 4 != 0, an unaligned y, and z as an NCHW view (z.sc != 1)."""
    i = [1, 5, 17].index(co)
    shp = [(7, 9, 20, 13), (11, 4, 61, 8), (9, 7, 4, 3)][i]
    run(case(2, *shp, co, bool(i & 1), ACTS[(2 * i + len(zk)) % 6]), ("fused", 1, 4), zk=zk, yk=yk)


@gpu
@pytest.mark.parametrize("co", [8, 5])
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("shp", FUSED_GEOM)
def test_fused_geometry(shp, ac, co):
    """Downsampling (the full-rebuild branch), identity, degenerate sizes (scale = 0 at Ho = 1 / Wo = 1), awkward
    ratios, Ho = 260. Identity at Co = 8 is the fused kernel with align_corners too (Co > 4)."""
    i = FUSED_GEOM.index(shp)
    run(case(2, *shp, co, ac, ACTS[(i + co) % 6]), ("fused", 4 if co == 8 else 1, 4),
        zk=("dense", "inner" if co == 8 else "odd")[i % 2], yk=("dense", "inner", "nchw")[i % 3])


@gpu
@pytest.mark.parametrize("R,N,Hi,Wi,Ho,Wo", LONG_R)
def test_fused_long_row_ranges(R, N, Hi, Wi, Ho, Wo):
    """The host keeps R only when N ceil(Ho / R) chunks >= 8192: Co = 1, Wo = 65536 (chunks = 256) and N = 11 give
    R = 8 at Ho = 17 and R = 16 at Ho = 33, three row blocks each, the last one ragged (1 row)."""
    run(case.__wrapped__(N, Hi, Wi, Ho, Wo, 1, True, "none"), ("fused", 1, R))     # not kept: 12 / 24 M outputs


@gpu
@pytest.mark.parametrize("zscale", [50.0, 1e-3])
def test_fused_data_scale(zscale):
    run(case(2, 7, 9, 20, 13, 24, False, "gelu", zscale), ("fused", 4), planes=True)
    run(case(2, 11, 4, 61, 8, 17, True, "silu", zscale), ("fused", 1), yk="odd")


# ====================================================================== separable form
@gpu
@pytest.mark.parametrize("yk", ["dense", "inner", "nchw"])
@pytest.mark.parametrize("co", [24, 5, 32, 17])
@pytest.mark.parametrize("shp,ac", [((7, 9, 20, 13), False), ((9, 7, 4, 3), True), ((4, 4, 20, 33), True)])
def test_separable_against_fp64(shp, ac, co, yk):
    """upconv_h_kernel / upconv_out_kernel <4> and <1>, otherwise only ever the reference of the bit checks."""
    vw = 4 if co % 4 == 0 else 1
    run(case(2, *shp, co, ac, ACTS[(co + len(yk)) % 6]), ("sep", vw), zk="inner" if vw == 4 else "odd", yk=yk,
        separable=True)


@gpu
@pytest.mark.parametrize("zscale", [50.0, 1e-3])
def test_separable_data_scale(zscale):
    run(case(2, 7, 9, 20, 13, 24, False, "gelu", zscale), ("sep", 4), separable=True)
    run(case(2, 11, 4, 61, 8, 17, True, "silu", zscale), ("sep", 1), yk="odd", separable=True)


@gpu
def test_separable_refuses_y_amax():
    c = case(2, 7, 9, 20, 13, 24, False, "gelu")
    y = Out(2, 20, 13, 24, "inner")
    ya = torch.zeros(2, device=DEV)
    with pytest.raises(PrpeError):
        launch(c, z_dev(c, "dense"), y.view, separable=True, ya=ya)
    torch.cuda.synchronize()
    assert y.untouched() and bool((y.cpu() == SENT).all()) and bool((ya.cpu() == 0).all())


# ====================================================================== host
def raw_call(c, z, y, ws_ptr, ws_bytes, planes=False, ya=None):
    sc, bi, sl = dptr(c.sc), dptr(c.bi), dptr(c.sl)
    zv, yv = ops.view(z), ops.view(y)
    st = lib().prpe_upconv3x3(C.byref(zv), C.byref(yv), 1 if c.ac else 0, ops._ptr(sc), ops._ptr(bi), ops._ptr(sl),
                              ACT[c.act], int(planes), ops._ptr(ya), ws_ptr, ws_bytes, ops._stream())
    torch.cuda.synchronize()
    return st


@gpu
@pytest.mark.parametrize("co,route", [(24, ("fused", 4)), (32, ("dma",)), (5, ("fused", 1))])
@pytest.mark.parametrize("how", ["short", "misaligned", "exact"])
def test_workspace_fall_through(how, co, route):
    """A workspace one byte short, or 4 bytes off the 16-byte grid, is not used: the one-pass route runs (same
    bits) and the workspace is never written. The exact, aligned one is used (and written)."""
    c = case(2, 4, 4, 20, 40, co, True, "gelu", seed=7)
    z, y = z_dev(c, "dense"), Out(2, 20, 40, co, "dense")
    assert route_of(z, y.view, True)[:len(route)] == route
    need = lib().prpe_upconv3x3_workspace_bytes(C.byref(ops.view(z)), C.byref(ops.view(y.view)))
    assert need == 4 * 3 * 2 * 4 * 40 * co
    ws = Guarded((need // 4 + 4,))
    base = ws.view.data_ptr()
    assert base % 16 == 0
    ptr, nb = {"short": (base, need - 1), "misaligned": (base + 4, need), "exact": (base, need)}[how]
    assert raw_call(c, z, y.view, ptr, nb) == 0
    got = y.cpu()
    held("separable" if how == "exact" else fam_of(route), f"workspace {how} Co{co}", c, got)
    assert same_bits(got, sep_bits(c)) and y.untouched()
    assert bool((ws.buf.cpu() == SENT).all()) == (how != "exact")


@gpu
@pytest.mark.parametrize("why", ["z.n", "z.c", "prelu-no-slope", "planes-co%8", "planes-misaligned", "planes-strided",
                                 "planes-nchw", "planes-workspace", "amax-workspace"])
def test_einval_leaves_buffers(why):
    """PRPE_EINVAL and nothing written to y, the slots or the workspace."""
    co = 12 if why == "planes-co%8" else 24
    c = case(2, 7, 9, 20, 13, co, False, "prelu" if why == "prelu-no-slope" else "gelu")
    z = z_dev(c, "dense")
    if why == "z.n":
        z = dev_in(torch.cat([c.z, c.z[:1]]))
    if why == "z.c":
        z = dev_in(c.z[..., :9 * co - 9].contiguous())
    yk = {"planes-misaligned": "inner", "planes-strided": "inner", "planes-nchw": "nchw"}.get(why, "dense")
    y = Out(2, 20, 13, co, yk)
    if why == "planes-misaligned":                       # dense strides, base 16 bytes off the 32-byte grid
        y.g = Guarded((2, 20, 13, co), None, 4)
        y.view = y.g.view
    planes = why.startswith("planes")
    ws = Guarded((3 * 2 * 7 * 13 * co + 4,))
    use_ws = why.endswith("workspace")
    ya = torch.zeros(2, device=DEV) if why == "amax-workspace" else None
    if why == "prelu-no-slope":
        c = SimpleNamespace(**{**vars(c), "sl": None})
    st = raw_call(c, z, y.view, ws.view.data_ptr() if use_ws else None, (ws.view.numel() - 4) * 4 if use_ws else 0,
                  planes, ya)
    assert st != 0
    assert y.untouched() and bool((y.g.buf.cpu() == SENT).all())
    assert bool((ws.buf.cpu() == SENT).all())
    assert ya is None or bool((ya.cpu() == 0).all())
