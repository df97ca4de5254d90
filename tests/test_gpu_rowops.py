"""GPU: the per-pixel, row and PSA kernels around the convolutions at every dispatch branch.

csrc/pointwise.hip (layernorm, l2norm, DFL decode, dwconv, maxpool, nearest 2x upsample, copy_pad,
norm_sigmoid), csrc/attention.hip (the two PSA kernels) and csrc/evalsteps.hip (flip_average,
ce_argmax), each against an fp64 torch restatement of the operation written here, or against the
fp32 torch op bit for bit where the operation is exact.

Every output lives in a buffer filled with a sentinel, with a margin of sentinel floats before and
after the view and, for strided views, between its rows / pixels; after the launch every float
outside the view must still hold the sentinel (``Guarded.untouched``). An element inside the view
that the kernel skipped still holds the sentinel too, and fails the value comparison.

Tolerances: the ones the suite already uses at unit-scale inputs (layernorm 1e-5, PSA 1e-5, DFL
rtol 2e-6 / atol 2e-5, l2norm rtol 1e-6 / atol 1e-7, dwconv 1e-5, cross-entropy rtol 1e-6 / atol
1e-5, norm_sigmoid 2e-6). Where a case changes the scale of the data (``scaled_tol``) the kernel
is allowed 4 times the largest distance between the fp32 torch CPU evaluation of the same inputs
and the fp64 reference: the factor covers another legitimate fp32 summation order and libm, and
is far below what an index or tail error produces. The measured ratios are in the docstrings.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.model_ref import make_anchors
from prpe import ops
from prpe._lib import PrpeError, check, lib
from test_gpu_ops import _decode_planes

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0            # no reference value comes near it
MARGIN = 64               # floats before and after every view (256 B: keeps 16 / 32-byte alignment)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def uni(*shape, seed, scale=1.0):
    return (torch.rand(*shape, generator=gen(seed)) * 2 - 1) * scale


def nrm(*shape, seed):
    return torch.randn(*shape, generator=gen(seed))


class Guarded:
    """A device buffer full of ``fill`` and a strided view of it that starts ``shift`` elements
    past a 256-byte aligned address, with MARGIN elements before and after."""

    def __init__(self, size, stride=None, shift=0, fill=SENT, dtype=torch.float32):
        self.size = tuple(int(v) for v in size)
        if stride is None:
            stride = [1] * len(self.size)
            for i in range(len(self.size) - 2, -1, -1):
                stride[i] = stride[i + 1] * self.size[i + 1]
        self.stride = tuple(int(v) for v in stride)
        assert all(s > 0 for s in self.stride)
        span = 1 + sum((n - 1) * s for n, s in zip(self.size, self.stride))
        self.start = MARGIN + shift
        self.fill = fill
        self.buf = torch.full((self.start + span + MARGIN,), fill, device=DEV, dtype=dtype)
        self.view = torch.as_strided(self.buf, self.size, self.stride, self.start)

    def untouched(self):
        """True when every element outside the view still holds the fill value."""
        host = self.buf.cpu()
        inside = torch.zeros(host.numel(), dtype=torch.bool)
        torch.as_strided(inside, self.size, self.stride, self.start).fill_(True)
        return bool((host[~inside] == self.fill).all())

    def cpu(self):
        return self.view.cpu()


def dev_in(t, stride=None, shift=0):
    """``t`` on the device inside a NaN-filled buffer (a read outside the view poisons the result)."""
    g = Guarded(t.shape, stride, shift, fill=float("nan"), dtype=t.dtype)
    g.view.copy_(t.to(DEV))
    return g.view


def nhwc_layout(n, h, w, c, kind):
    """(stride, shift) of a logical NHWC view: dense, the interior of a larger NHWC buffer with 4
    more channels per pixel (16-byte alignment kept), the same with 5 more channels and an odd
    start (nothing aligned), a permuted NCHW tensor, or (concat) channels [8, 8 + c) of a dense
    NHWC buffer of c + 16 channels: pixels, rows and frames stay linear at a pixel stride > c."""
    if kind == "dense":
        return (h * w * c, w * c, c, 1), 0
    if kind == "nchw":
        return (c * h * w, w, 1, h * w), 0
    if kind == "concat":
        return (h * w * (c + 16), w * (c + 16), c + 16, 1), 8
    pc = 4 if kind == "inner" else 5
    sw = c + pc
    sh = (w + 2) * sw
    sn = (h + 3) * sh
    return (sn, sh, sw, 1), (sh + sw + 4 if kind == "inner" else sh + sw + 1)


def g_nhwc(n, h, w, c, kind="dense"):
    st, sf = nhwc_layout(n, h, w, c, kind)
    return Guarded((n, h, w, c), st, sf)


def in_nhwc(t_nchw, kind="dense"):
    """CPU NCHW tensor -> device logical-NHWC view in the given layout."""
    t = t_nchw.permute(0, 2, 3, 1)
    st, sf = nhwc_layout(*t.shape, kind)
    return dev_in(t, st, sf)


def to_nchw(g):
    return g.cpu().permute(0, 3, 1, 2)


def same_bits(a, b):
    """Equal values, NaN where and only where the other has NaN (torch.equal fails on NaN)."""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(torch.where(a.isnan(), torch.zeros_like(a), a), torch.where(b.isnan(), torch.zeros_like(b), b))


def scaled_tol(what, got, ref64, ref32):
    """4 x the largest distance of the fp32 torch CPU evaluation from the fp64 reference; prints
    the kernel's share of it, returns (kernel error, allowance)."""
    e32 = float((ref32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    print(f"\n{what}: kernel max err {err:.3e}  fp32 torch max err {e32:.3e}  ratio {err / e32 if e32 else 0.0:.3f}")
    return err, 4.0 * e32


# ====================================================================== 1. layernorm
LN_C = [4, 64, 252, 256, 260, 508, 512, 516, 768, 772, 1024, 1028, 770, 1, 63]


def ln_ref(x, g, b, eps, relu, dtype=torch.float64):
    r = F.layer_norm(x.to(dtype), (x.shape[1],), g.to(dtype), b.to(dtype), eps)
    return F.relu(r) if relu else r


def ln_params(C, seed):
    return torch.rand(C, generator=gen(seed)) + 0.5, uni(C, seed=seed + 1)


def ln_run(x, g, b, eps, relu, xs=None, ys=None, xshift=0, yshift=0, planes=False):
    rows, C = x.shape
    xd = dev_in(x, (xs or C, 1), xshift)
    y = Guarded((rows, C), (ys or C, 1), yshift)
    ops.layernorm(xd, y.view, g.to(DEV), b.to(DEV), eps, relu, planes)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("rows", [1, 3, 5, 7])
@pytest.mark.parametrize("C", LN_C)
def test_layernorm_every_kernel_and_row_tail(C, rows):
    """Each register kernel <1..4> at its lower edge, inside and at its upper edge (C = 4 .. 1024),
    the generic kernel (C % 4 != 0, C > 1024), and row counts that leave 1..3 idle waves in the last
    4-row block. relu and eps alternate over the grid (each value meets each kernel)."""
    i = LN_C.index(C)
    relu, eps = bool((i + rows // 2) & 1), (1e-12, 1e-5)[(i // 2 + rows // 4) & 1]
    x = nrm(rows, C, seed=100 + C)
    g, b = ln_params(C, 200 + C)
    y = ln_run(x, g, b, eps, relu)
    torch.testing.assert_close(y.cpu().double(), ln_ref(x, g, b, eps, relu), rtol=0, atol=1e-5)
    assert y.untouched()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("C", [256, 512, 768, 1024, 770])
def test_layernorm_relu_and_eps(C, eps, relu):
    x = nrm(5, C, seed=300 + C)
    g, b = ln_params(C, 310 + C)
    y = ln_run(x, g, b, eps, relu)
    torch.testing.assert_close(y.cpu().double(), ln_ref(x, g, b, eps, relu), rtol=0, atol=1e-5)
    assert y.untouched()


@pytest.mark.parametrize("mode", ["x+4", "y+4", "x+1", "y+2", "x@1", "y@1", "xy+4"])
@pytest.mark.parametrize("C", [64, 512, 772, 1024])
def test_layernorm_row_slices_and_misaligned_pointers(C, mode):
    """Rows as slices of a wider buffer: a stride of C + 4 keeps the float4 kernels, C + 1 / C + 2
    or a base one float off the 16-byte grid must take the generic kernel; either way the floats
    between the rows stay as they were."""
    kw = {"x+4": dict(xs=C + 4), "y+4": dict(ys=C + 4), "x+1": dict(xs=C + 1), "y+2": dict(ys=C + 2),
          "x@1": dict(xshift=1), "y@1": dict(yshift=1), "xy+4": dict(xs=C + 4, ys=C + 8)}[mode]
    x = nrm(5, C, seed=400 + C)
    g, b = ln_params(C, 410 + C)
    y = ln_run(x, g, b, 1e-12, True, **kw)
    torch.testing.assert_close(y.cpu().double(), ln_ref(x, g, b, 1e-12, True), rtol=0, atol=1e-5)
    assert y.untouched()


@pytest.mark.parametrize("C", [256, 512, 770, 1024])
def test_layernorm_mean_far_above_std(C):
    """Rows of 1000 + N(0, 1): the fp32 mean of C values near 1000 carries the error.

    Measured on the MI355X (kernel error / fp32 torch error): C = 256 0.62, 512 1.01, 770 0.77,
    1024 0.55 (errors of 6.6e-5 .. 9.8e-5 on outputs of a few units).
    """
    x = 1000.0 + nrm(5, C, seed=500 + C)
    g, b = ln_params(C, 510 + C)
    y = ln_run(x, g, b, 1e-5, False)
    err, tol = scaled_tol(f"layernorm 1000+N(0,1) C={C}", y.cpu(), ln_ref(x, g, b, 1e-5, False),
                          ln_ref(x, g, b, 1e-5, False, torch.float32))
    assert err <= tol
    assert y.untouched()


@pytest.mark.parametrize("relu", [False, True])
def test_layernorm_constant_row_gives_beta_exactly(relu):
    """C = 256 at 0.5: the sum (128) and the mean are exact, every centred value is 0, so the
    output is beta (its relu) bit for bit whatever 1 / sqrt(eps) is."""
    C = 256
    g, b = ln_params(C, 600)
    y = ln_run(torch.full((3, C), 0.5), g, b, 1e-12, relu)
    ref = (F.relu(b) if relu else b).expand(3, C)
    assert torch.equal(y.cpu(), ref)
    assert y.untouched()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", [256, 512, 1024])
def test_layernorm_planes_output(C, relu):
    """The planes output of <1>, <2> and <4> == the fp32 output of the same call split into
    hi = RNE(v), lo = RNE(v - hi), with a row tail (rows = 5)."""
    rows = 5
    x = nrm(rows, C, seed=700 + C) * 3.0
    g, b = ln_params(C, 710 + C)
    y32 = ln_run(x, g, b, 1e-12, relu)
    ypl = ln_run(x, g, b, 1e-12, relu, planes=True)
    v = y32.cpu().view(rows, 1, 1, C)
    hi, lo = _decode_planes(ypl.cpu().view(rows, 1, 1, C))
    assert torch.equal(hi, v.to(torch.bfloat16).float())
    assert torch.equal(lo, (v - hi).to(torch.bfloat16).float())
    assert y32.untouched() and ypl.untouched()


def test_layernorm_planes_refusals():
    for C, kw in ((252, {}), (1032, {}), (256, dict(yshift=4)), (256, dict(yshift=1)), (256, dict(ys=260))):
        g, b = ln_params(C, 800)
        with pytest.raises(PrpeError):
            ln_run(nrm(3, C, seed=801), g, b, 1e-12, False, planes=True, **kw)


# ====================================================================== 2. PSA attention
def psa_ref(qkv, nh, dk, dh):
    """qkv: CPU [B, nh * (2 dk + dh), h, w] -> (out, v) fp64 [B, nh * dh, h, w]."""
    B, _, h, w = qkv.shape
    t = qkv.reshape(B, nh, 2 * dk + dh, h * w).double()
    q, k, v = t.split([dk, dk, dh], dim=2)
    att = ((q.transpose(-2, -1) @ k) * dk ** -0.5).softmax(-1)
    return (v @ att.transpose(-2, -1)).reshape(B, nh * dh, h, w), v.reshape(B, nh * dh, h, w)


def psa_streams(h, w, nh):
    return nh * (h * w) ** 2 * 4 > 64 * 1024


def psa_check(qkv, nh, dk, dh, kind="dense", with_v=True):
    B, _, h, w = qkv.shape
    out = g_nhwc(B, h, w, nh * dh, kind)
    vout = g_nhwc(B, h, w, nh * dh, kind) if with_v else None
    ops.psa_attention(in_nhwc(qkv, kind), out.view, vout.view if with_v else None, nh, dk, dh, dk ** -0.5)
    torch.cuda.synchronize()
    ref, v = psa_ref(qkv, nh, dk, dh)
    torch.testing.assert_close(to_nchw(out).double(), ref, rtol=0, atol=1e-5)
    assert out.untouched()
    if with_v:
        assert torch.equal(to_nchw(vout), v.float())
        assert vout.untouched()


PSA_MAPS = [
    (3, 7, 2, False),      # LDS kernel, non-square
    (9, 10, 2, False),     # L = 90: 64,800 B of scores, the last size in LDS at nh = 2
    (7, 13, 2, True),      # L = 91: the first size that streams
    (13, 23, 2, True),     # L = 299: second query block of 43 threads, last key chunk of 43
    (8, 16, 1, False),     # nh = 1 moves the edge to L = 128 (exactly 64 KiB)
    (3, 43, 1, True),      # L = 129
    (7, 10, 3, False),     # nh = 3: L = 70 fits
    (2, 37, 3, True),      # nh = 3: L = 74 streams
]


@pytest.mark.parametrize("h,w,nh,streams", PSA_MAPS)
def test_psa_attention_non_square_maps_both_sides_of_the_switch(h, w, nh, streams):
    """Tokens are (i / W, i % W): on a non-square map a swapped h and w reads other pixels."""
    assert psa_streams(h, w, nh) == streams
    psa_check(uni(2, nh * 128, h, w, seed=1000 + h * w), nh, 32, 64)


@pytest.mark.parametrize("h,w", [(3, 7), (7, 13)])
@pytest.mark.parametrize("dh", [16, 64])
@pytest.mark.parametrize("dk", [8, 32])
def test_psa_attention_narrow_heads(h, w, dk, dh):
    """dk < 32 / dh < 64: the streaming kernel's zero-filled key and value columns."""
    psa_check(uni(2, 2 * (2 * dk + dh), h, w, seed=1100 + dk + dh + h), 2, dk, dh)


@pytest.mark.parametrize("h,w", [(3, 7), (13, 23)])
@pytest.mark.parametrize("kind,with_v", [("dense", False), ("inner", True), ("inner", False), ("odd", True)])
def test_psa_attention_views_and_no_vout(h, w, kind, with_v):
    """vout = None; qkv, out and vout as channel slices of wider buffers."""
    psa_check(uni(2, 2 * 128, h, w, seed=1200 + h), 2, 32, 64, kind, with_v)


@pytest.mark.parametrize("h,w", [(9, 10), (13, 23)])
def test_psa_attention_adversarial_rows(h, w):
    """A key that dominates late in the walk (the last key, and one in the last ragged chunk), a
    dominant first key, and a query whose logits are all equal (uniform weights). The output stays
    a convex combination of unit-scale values, so the unit-scale tolerance holds."""
    B, nh, dk, dh = 2, 2, 32, 64
    L = h * w
    qkv = uni(B, nh * 128, h, w, seed=1300 + h)
    t = qkv.view(B, nh, 128, L)
    for n, hd, i, j in ((0, 0, 3, L - 1), (0, 1, L - 1, L - 20), (1, 0, L // 2, 0), (1, 1, 0, L // 2)):
        qi = t[n, hd, :dk, i]
        t[n, hd, dk:2 * dk, j] = qi * (40.0 * dk ** 0.5 / float(qi @ qi))       # logit (i, j) = 40
    t[1, 1, :dk, 11] = 0.0
    psa_check(qkv, nh, dk, dh)


def test_psa_attention_refusals():
    h, w, nh = 7, 13, 2
    assert psa_streams(h, w, nh)
    for dk, dh in ((40, 64), (32, 80)):
        qkv = uni(1, h, w, nh * (2 * dk + dh), seed=1400).to(DEV)
        with pytest.raises(PrpeError):
            ops.psa_attention(qkv, torch.empty(1, h, w, nh * dh, device=DEV), None, nh, dk, dh, dk ** -0.5)
    qkv = uni(1, h, w, nh * 128, seed=1401).to(DEV)
    out = torch.empty(1, h, w, nh * 64, device=DEV)
    for shape in ((1, w, h, nh * 64), (1, h, w - 1, nh * 64), (1, h, w, nh * 64 - 4)):
        with pytest.raises(PrpeError):
            ops.psa_attention(qkv, torch.empty(*shape, device=DEV), None, nh, 32, 64, 32 ** -0.5)
        with pytest.raises(PrpeError):
            ops.psa_attention(qkv, out, torch.empty(*shape, device=DEV), nh, 32, 64, 32 ** -0.5)


# ====================================================================== 3. DFL decode
def dfl_ref(head, nc, levels, strides, dtype=torch.float64):
    """The head's eval decode (softmax expectation over 16 bins, anchors, strides, sigmoid)."""
    B, A, _ = head.shape
    feats = [torch.zeros(1, 1, h, w, dtype=dtype) for h, w in levels]
    anchors, st = (t.transpose(0, 1) for t in make_anchors(feats, strides))
    box, cls = head.to(dtype).transpose(1, 2).split((64, nc), 1)
    d = box.reshape(B, 4, 16, A).transpose(2, 1).softmax(1)
    d = (d * torch.arange(16, dtype=dtype).view(1, 16, 1, 1)).sum(1)
    lt, rb = d.chunk(2, 1)
    a1, b1 = anchors.unsqueeze(0) - lt, anchors.unsqueeze(0) + rb
    return torch.cat((torch.cat(((a1 + b1) / 2, b1 - a1), 1) * st, cls.sigmoid()), 1)


def dfl_run(head, nc, levels, strides):
    B, A, _ = head.shape
    out = Guarded((B, 4 + nc, A))
    ops.dfl_decode(dev_in(head), out.view, nc, levels, strides)
    torch.cuda.synchronize()
    return out


DFL_LEVELS = [[(8, 6), (4, 3), (2, 2)], [(5, 9)], [(4, 4), (3, 5), (2, 2), (1, 3)]]
DFL_IDS = ["3lev", "1lev", "4lev"]
PIXEL_STRIDES = [8.0, 16.0, 32.0, 64.0]


def dfl_check_scaled(what, out, head, nc, levels, strides):
    """Box rows level by level under the 4 x fp32-torch rule (the stride scales the expectation, whose
    fp32 resolution is 2^-20 at 8..15 bins, to 6e-5 px at stride 64: above the unit-scale atol); the
    class rows keep the unit-scale tolerance."""
    r64, r32 = dfl_ref(head, nc, levels, strides), dfl_ref(head, nc, levels, strides, torch.float32)
    got, a0 = out.cpu(), 0
    for (h, w), st in zip(levels, strides):
        sl = slice(a0, a0 + h * w)
        err, tol = scaled_tol(f"{what} level {h}x{w} stride {st:g}", got[:, :4, sl], r64[:, :4, sl], r32[:, :4, sl])
        assert err <= tol
        a0 += h * w
    torch.testing.assert_close(got[:, 4:].double(), r64[:, 4:], rtol=2e-6, atol=2e-5)
    assert out.untouched()


@pytest.mark.parametrize("stride", [0.0, 1.0])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("nc", [1, 3, 80])
@pytest.mark.parametrize("levels", DFL_LEVELS, ids=DFL_IDS)
def test_dfl_decode_levels_classes_batches(levels, nc, B, stride):
    """Non-square levels (the anchor is (ia % w, ia / w)), 1, 3 and 4 levels, the (4 + c) * A class
    rows, B * A below 256 (64, 192; 45 .. 225; 38 .. 190) and above it but no multiple (320: a
    second block of 64 live threads). Zero strides (a fresh head: every box row 0) and unit strides
    (boxes in grid cells, the unit scale of the tolerance)."""
    A = sum(h * w for h, w in levels)
    strides = [stride] * len(levels)
    head = uni(B, A, 64 + nc, seed=2000 + A + nc, scale=3.0)
    out = dfl_run(head, nc, levels, strides)
    torch.testing.assert_close(out.cpu().double(), dfl_ref(head, nc, levels, strides), rtol=2e-6, atol=2e-5)
    assert out.untouched()


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("nc", [1, 80])
@pytest.mark.parametrize("levels", DFL_LEVELS, ids=DFL_IDS)
def test_dfl_decode_pixel_strides(levels, nc, B):
    """Strides 8, 16, 32, 64: each level must take its own stride.

    Measured on the MI355X (kernel error / fp32 torch error, per level): 0.61 .. 1.71 over the 48
    levels of the 18 cases (the largest at the 1x3 level of stride 64, B = 1: 12 numbers). The
    unit-scale atol of 2e-5 does not hold here: 2.8e-5 .. 5.0e-5 px at strides 32 and 64, where the
    fp32 torch decode is as far from fp64.
    """
    A = sum(h * w for h, w in levels)
    strides = PIXEL_STRIDES[:len(levels)]
    head = uni(B, A, 64 + nc, seed=2000 + A + nc, scale=3.0)
    dfl_check_scaled(f"dfl A={A} nc={nc} B={B}", dfl_run(head, nc, levels, strides), head, nc, levels, strides)


@pytest.mark.parametrize("levels", DFL_LEVELS, ids=DFL_IDS)
def test_dfl_decode_saturated_bins(levels):
    """One bin of a side at +80 (the softmax is that bin) or at -80 (that bin vanishes) on two
    anchors in three, the other logits at scale 3; pixel strides.

    Measured on the MI355X (kernel error / fp32 torch error, per level): 0.75 .. 1.01 over the 8
    levels.
    """
    B, nc = 3, 3
    A = sum(h * w for h, w in levels)
    strides = PIXEL_STRIDES[:len(levels)]
    head = uni(B, A, 64 + nc, seed=2100 + A, scale=3.0)
    bins = torch.randint(0, 64, (B, A), generator=gen(2101))
    for b in range(B):
        for a in range(A):
            if a % 3 < 2:
                head[b, a, bins[b, a]] = 80.0 if a % 3 == 0 else -80.0
    dfl_check_scaled(f"dfl +-80 A={A}", dfl_run(head, nc, levels, strides), head, nc, levels, strides)


# ====================================================================== 4. dwconv
def act64(v, act):
    return {"none": lambda t: t, "relu": F.relu, "silu": F.silu, "gelu": F.gelu, "sigmoid": torch.sigmoid}[act](v)


def dw_case(B, C, H, W, k, s, p, act="silu", scale=True, bias=True, res=True, xk="dense", yk="dense", rk="dense",
            seed=3000):
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = uni(B, C, H, W, seed=seed)
    w = uni(C, 1, k, k, seed=seed + 1) / k                       # |sum| stays O(1) at every k
    sc = torch.rand(C, generator=gen(seed + 2)) + 0.5 if scale else None
    bi = uni(C, seed=seed + 3) if bias else None
    r = uni(B, C, Ho, Wo, seed=seed + 4) if res else None
    y = g_nhwc(B, Ho, Wo, C, yk)
    ops.dwconv(in_nhwc(x, xk), y.view, dev_in(w.reshape(-1)), k, s, p, None if sc is None else dev_in(sc),
               None if bi is None else dev_in(bi), act, res=None if r is None else in_nhwc(r, rk))
    torch.cuda.synchronize()
    ref = F.conv2d(x.double(), w.double(), None, s, p, 1, C)
    if scale:
        ref = ref * sc.double().view(1, -1, 1, 1)
    if bias:
        ref = ref + bi.double().view(1, -1, 1, 1)
    ref = act64(ref, act)
    if res:
        ref = ref + r.double()
    torch.testing.assert_close(to_nchw(y).double(), ref, rtol=0, atol=1e-5)
    assert y.untouched()


@pytest.mark.parametrize("C", [1, 5, 80])
@pytest.mark.parametrize("H,W", [(7, 11), (10, 10), (1, 9)])
@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2), (1, 1, 0)])
def test_dwconv_geometries(k, s, p, H, W, C):
    """Stride 2, k = 1 / 3 / 5, H != W, a one-row map; 7x11 and 10x10 at C = 80 put several
    256-thread chunks on one output row."""
    if C == 80 and s == 1:
        assert ((W + 2 * p - k) // s + 1) * C > 256
    dw_case(2, C, H, W, k, s, p, act=("silu", "relu", "none")[(k + s + C) % 3], seed=3000 + 7 * k + s + C + H)


@pytest.mark.parametrize("scale,bias,res", [(False, True, True), (True, False, True), (True, True, False),
                                            (False, False, False)])
def test_dwconv_optional_operands(scale, bias, res):
    dw_case(2, 5, 7, 11, 3, 2, 1, "silu", scale, bias, res, seed=3100)


@pytest.mark.parametrize("act", ["none", "relu", "silu", "gelu", "sigmoid"])
def test_dwconv_activations(act):
    dw_case(2, 80, 7, 11, 3, 1, 1, act, seed=3200)


def test_dwconv_refuses_prelu():
    x = uni(1, 4, 4, 8, seed=3300).to(DEV)
    with pytest.raises(PrpeError):
        ops.dwconv(x, torch.empty_like(x), uni(8 * 9, seed=3301).to(DEV), 3, 1, 1, None, None, "prelu")


@pytest.mark.parametrize("xk,yk,rk", [("inner", "inner", "inner"), ("odd", "nchw", "odd"), ("nchw", "odd", "dense")])
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (5, 1, 2)])
def test_dwconv_strided_views(k, s, p, xk, yk, rk):
    """x, y and the residual as interior views of larger buffers, NCHW-permuted views."""
    dw_case(2, 5, 7, 11, k, s, p, "silu", xk=xk, yk=yk, rk=rk, seed=3400 + k)


# ====================================================================== 5. maxpool
@pytest.mark.parametrize("data", ["negative", "inf_nan"])
@pytest.mark.parametrize("C,xk,yk", [(16, "dense", "dense"), (16, "inner", "inner"), (6, "dense", "dense"),
                                     (16, "odd", "dense"), (16, "dense", "odd"), (6, "nchw", "inner")])
@pytest.mark.parametrize("H,W", [(33, 20), (5, 7), (14, 9)])
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (5, 1, 2), (2, 2, 0), (1, 2, 0)])
def test_maxpool_both_kernels_bit_exact(k, s, p, H, W, C, xk, yk, data):
    """The float4 kernel (C = 16, aligned views) and the scalar one (C = 6, or C = 16 through a view
    one float off the 16-byte grid), H != W, windows that hang over the top / left edge only, sizes
    whose last rows and columns no window reaches. All-negative maps show a zero used as padding;
    -inf and NaN must come out as F.max_pool2d gives them."""
    B = 2
    x = -0.01 - torch.rand(B, C, H, W, generator=gen(4000 + H + k))
    if data == "inf_nan":
        m = torch.rand(B, C, H, W, generator=gen(4001 + H + k))
        x[m < 0.25] = float("-inf")
        x[m > 0.97] = float("nan")
        x[0, 0] = float("-inf")                                  # whole windows of -inf
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = g_nhwc(B, Ho, Wo, C, yk)
    ops.maxpool(in_nhwc(x, xk), y.view, k, s, p)
    torch.cuda.synchronize()
    assert same_bits(to_nchw(y), F.max_pool2d(x, k, s, p))
    assert y.untouched()


# ====================================================================== 6. nearest 2x upsample
@pytest.mark.parametrize("xk,yk", [("dense", "dense"), ("inner", "inner"), ("nchw", "odd")])
@pytest.mark.parametrize("C", [1, 8, 130])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (7, 2)])
def test_upsample_nearest2x_bit_exact(H, W, C, xk, yk):
    """1x1, H != W, and rows of more than 256 (pixel, channel) pairs (2 W C = 520 .. 1300)."""
    B = 2
    x = uni(B, C, H, W, seed=5000 + H + C)
    y = g_nhwc(B, 2 * H, 2 * W, C, yk)
    ops.upsample_nearest2x(in_nhwc(x, xk), y.view)
    torch.cuda.synchronize()
    assert torch.equal(to_nchw(y), F.interpolate(x, scale_factor=2.0, mode="nearest"))
    assert y.untouched()


# ====================================================================== 7. l2norm
def l2_ref(x, eps, dtype=torch.float64):
    n = torch.norm(x.to(dtype), 2, 1, True)
    return x.to(dtype) / n.clamp_min(eps), n


def l2_run(x, eps):
    rows, C = x.shape
    emb, nr = Guarded((rows, C)), Guarded((rows, 1))
    ops.l2norm(dev_in(x), emb.view, nr.view, eps)
    torch.cuda.synchronize()
    return emb, nr


@pytest.mark.parametrize("eps", [0.0, 1e-12])
@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("C", [1, 7, 63, 64, 65, 512, 1000])
def test_l2norm_widths_and_row_tail(C, rows, eps):
    """C < 64 (idle lanes), C not a multiple of 64, rows that leave idle waves in the last block."""
    x = uni(rows, C, seed=6000 + C + rows)
    emb, nr = l2_run(x, eps)
    re, rn = l2_ref(x, eps)
    torch.testing.assert_close(nr.cpu().double(), rn, rtol=1e-6, atol=0)
    torch.testing.assert_close(emb.cpu().double(), re, rtol=1e-6, atol=1e-7)
    assert emb.untouched() and nr.untouched()


@pytest.mark.parametrize("eps", [0.0, 1e-12])
@pytest.mark.parametrize("scale", [1e-18, 1e18])
@pytest.mark.parametrize("C", [7, 64, 1000])
def test_l2norm_extreme_scales(C, scale, eps):
    """Rows at 1e-18 (squares near the smallest normal fp32: an fp32 sum of squares loses bits or
    underflows) and at 1e18 (squares of 1e36: at C = 1000 their fp32 sum is at the edge of overflow).
    The kernel sums squares in fp64, so the embedding, which is scale-free, also keeps the unit-scale
    tolerance; the norm is compared relatively (1e-6), and in units of the scale. With eps = 1e-12
    the rows at 1e-18 are divided by the clamp, not by their norm.

    Measured on the MI355X (kernel error / fp32 torch error): embedding 0.86 .. 1.00 and norm
    0.69 .. 1.00 wherever the fp32 torch norm is finite; at 1e18 and C = 1000 it overflows (its
    embedding is 5.4e-2 off, its norm 18 units of the scale) and the kernel stays at 3.4e-9 / 5.2e-7.
    """
    x = uni(3, C, seed=6100 + C) * scale
    emb, nr = l2_run(x, eps)
    re, rn = l2_ref(x, eps)
    re32, rn32 = l2_ref(x, eps, torch.float32)
    err, tol = scaled_tol(f"l2norm emb C={C} x{scale:g} eps={eps:g}", emb.cpu(), re, re32.nan_to_num(0.0, 0.0, 0.0))
    assert err <= tol
    err, tol = scaled_tol(f"l2norm norm/scale C={C} x{scale:g}", nr.cpu().double() / scale, rn / scale,
                          rn32.double().nan_to_num(0.0, 0.0, 0.0) / scale)
    assert err <= tol
    torch.testing.assert_close(emb.cpu().double(), re, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(nr.cpu().double(), rn, rtol=1e-6, atol=0)
    assert emb.untouched() and nr.untouched()


# ====================================================================== 8. ce_argmax
def ce_run(logits, labels, ld_pad=0, want_summary=True):
    """prpe_ce_argmax on a column slice of a [B, C + ld_pad] matrix; guarded loss / argmax /
    summary buffers. Returns (loss, amax, summary) Guarded (None where not asked for)."""
    B, Cn = logits.shape
    x = dev_in(logits, (Cn + ld_pad, 1))
    amax = Guarded((B,), dtype=torch.int32)
    loss = summary = lab = None
    if labels is not None:
        lab = labels.to(device=DEV, dtype=torch.int64)
        loss = Guarded((B,))
        summary = Guarded((2,)) if want_summary else None
    p = lambda g: None if g is None else g.view.data_ptr()
    check(lib().prpe_ce_argmax(x.data_ptr(), x.stride(0), B, Cn, None if lab is None else lab.data_ptr(), p(loss),
                               p(amax), p(summary), ops._stream()), "prpe_ce_argmax")
    torch.cuda.synchronize()
    return loss, amax, summary


def ce_check(logits, labels, loss, amax, summary):
    B = logits.shape[0]
    ref_rows = F.cross_entropy(logits.double(), labels, reduction="none")
    ref_amax = logits.max(1)[1]
    assert torch.equal(amax.cpu().long(), ref_amax)
    torch.testing.assert_close(loss.cpu().double(), ref_rows, rtol=1e-6, atol=1e-5, equal_nan=True)
    s = summary.cpu()
    m = ref_rows.mean()
    if torch.isnan(m) or torch.isinf(m):
        assert same_bits(s[0:1].double(), m.float().double().view(1))
    else:
        torch.testing.assert_close(s[0:1].double(), m.view(1), rtol=1e-6, atol=1e-5)
    assert s[1].item() == float(np.float32(int((ref_amax == labels).sum()) / B))
    assert loss.untouched() and amax.untouched() and summary.untouched()


@pytest.mark.parametrize("B", [1, 37, 300])
@pytest.mark.parametrize("C", [1, 2, 63, 255, 256, 257, 1000])
def test_ce_argmax_widths_batches_and_leading_dimension(C, B):
    """C < 256 (threads with no column), C around one block's stride, B > 256 (the summary kernel
    strides over the rows), ld = C and ld = C + 3. Labels hit the argmax on about half the rows."""
    logits = nrm(B, C, seed=7000 + C + B) * 5
    labels = torch.randint(0, C, (B,), generator=gen(7001 + C + B))
    hit = torch.rand(B, generator=gen(7002 + C)) < 0.5
    labels[hit] = logits.max(1)[1][hit]
    ce_check(logits, labels, *ce_run(logits, labels, ld_pad=3 * ((C + B) & 1)))


@pytest.mark.parametrize("C", [63, 257, 1000])
def test_ce_argmax_ties_last_column_nan_and_inf_rows(C):
    """Equal maxima at c = 5 and c = 5 + 64 k (other waves, other loop passes): the first wins. The
    maximum in the last column. NaN counts as the maximum, the first NaN wins. A row of -inf
    gives index 0 as torch.max does (every thread's (-inf, first column) against the idle threads'
    (-inf, none)); a row whose only finite logit is its label."""
    logits = nrm(9, C, seed=7100 + C) * 5
    ties = [c for c in (5, 5 + 64, 5 + 128, 5 + 192, 5 + 256, 5 + 640) if c < C]
    logits[0, ties] = 50.0
    logits[1, C - 1] = 60.0
    logits[2, C // 2] = float("nan")
    logits[2, 3] = 70.0
    logits[3] = float("-inf")
    logits[4, [C - 2, 7]] = float("nan")
    logits[5] = float("-inf")
    logits[5, C - 3] = 1.5
    logits[6] = float("-inf")
    logits[6, 2] = -4.0
    logits[7, [0, C - 1]] = 55.0
    labels = torch.tensor([5, C - 1, 3, 0, 7, C - 3, 1, 0, 4])
    loss, amax, summary = ce_run(logits, labels, ld_pad=3)
    assert amax.cpu().tolist()[:8] == [5, C - 1, C // 2, 0, 7, C - 3, 2, 0]
    assert loss.cpu()[6].item() == float("inf")
    ce_check(logits, labels, loss, amax, summary)


@pytest.mark.parametrize("C", [1, 2, 255, 256, 257])
def test_ce_argmax_all_minus_inf_rows(C):
    logits = torch.full((3, C), float("-inf"))
    loss, amax, summary = ce_run(logits, torch.zeros(3, dtype=torch.int64))
    assert amax.cpu().tolist() == [0, 0, 0]
    assert bool(loss.cpu().isnan().all())
    assert loss.untouched() and amax.untouched() and summary.untouched()


@pytest.mark.parametrize("C", [63, 1000])
def test_ce_argmax_large_logits(C):
    """Logits near 1e4: exp overflows fp32 unless the maximum is subtracted first.

    Measured on the MI355X (kernel error / fp32 torch error): rows 1.00 at both widths (2.9e-6,
    3.8e-6: both are the fp64 value rounded to fp32); mean 1.00 at C = 63, 0.18 at C = 1000.
    """
    B = 37
    logits = 1e4 + nrm(B, C, seed=7200 + C) * 20
    labels = torch.randint(0, C, (B,), generator=gen(7201 + C))
    loss, amax, summary = ce_run(logits, labels)
    ref = F.cross_entropy(logits.double(), labels, reduction="none")
    err, tol = scaled_tol(f"ce 1e4 C={C}", loss.cpu(), ref, F.cross_entropy(logits, labels, reduction="none"))
    assert err <= tol
    assert bool(torch.isfinite(loss.cpu()).all())
    assert torch.equal(amax.cpu().long(), logits.max(1)[1])
    err, tol = scaled_tol(f"ce 1e4 C={C} mean", summary.cpu()[0:1], ref.mean().view(1),
                          F.cross_entropy(logits, labels).view(1))
    assert err <= tol
    assert loss.untouched() and amax.untouched() and summary.untouched()


@pytest.mark.parametrize("C", [63, 257])
def test_ce_argmax_without_labels(C):
    logits = nrm(37, C, seed=7300 + C) * 5
    loss, amax, summary = ce_run(logits, None, ld_pad=3)
    assert loss is None and summary is None
    assert torch.equal(amax.cpu().long(), logits.max(1)[1])
    assert amax.untouched()
    l2, a2, s2 = ops.ce_argmax(logits.to(DEV))
    assert l2 is None and s2 is None and torch.equal(a2.cpu().long(), logits.max(1)[1])


# ====================================================================== 9. flip_average
def flip_ref(heat, flipped, partner, mode):
    """(heat + flip-back) / 2: the flipped pass mirrored along W; a paired joint takes the batch
    reversal of its own channel (mode 0, the reference's ``[:, pair].flip(0)``) or its partner's
    channel (mode 1)."""
    f = flipped.flip(-1)
    back = f.clone()
    for k, p in enumerate(partner):
        if p >= 0:
            back[:, k] = f.flip(0)[:, k] if mode == 0 else f[:, p]
    return (heat + back) * 0.5


def pair_table(K):
    """Joint 0 unpaired, then (1, 2), (3, 4), ...; a last joint without a partner stays unpaired.
    K = 1: the joint is its own partner, so the paired branch still runs."""
    if K == 1:
        return [0]
    t = [-1] * K
    for a in range(1, K - 1, 2):
        t[a], t[a + 1] = a + 1, a
    return t


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,K,H", [(1, 1, 1), (2, 17, 3), (3, 64, 1), (1, 17, 3)])
@pytest.mark.parametrize("W", [1, 2, 47, 255, 256, 257])
def test_flip_average_bit_exact_both_launch_widths(W, B, K, H, mode):
    """W < 256 runs 64 threads per row, W >= 256 runs 256; odd W has a centre column that maps to
    itself; B = 1 in the reference mode reverses a batch of one."""
    heat = torch.rand(B, K, H, W, generator=gen(8000 + W + K))
    flipped = torch.rand(B, K, H, W, generator=gen(8001 + W + K))
    partner = pair_table(K)
    out = Guarded((B, K, H, W))
    pa = (C.c_int32 * K)(*partner)
    hd, fd = dev_in(heat), dev_in(flipped)
    check(lib().prpe_flip_average(hd.data_ptr(), fd.data_ptr(), out.view.data_ptr(), B, K, H, W, pa, mode,
                                  ops._stream()), "prpe_flip_average")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), flip_ref(heat, flipped, partner, mode))
    assert out.untouched()


def test_flip_average_refuses_more_joints_than_the_table_holds():
    h = torch.rand(1, 65, 2, 2, device=DEV)
    with pytest.raises(PrpeError):
        ops.flip_average(h, h.clone(), [-1] * 65, 0)


# ====================================================================== 10. copy_pad, norm_sigmoid
@pytest.mark.parametrize("xc,yc", [(3, 4), (3, 3), (3, 5), (1, 4)])
@pytest.mark.parametrize("H,W", [(13, 21), (12, 21), (13, 300), (12, 300)])
def test_copy_pad_rows_per_block_and_amax(H, W, xc, yc):
    """Blocks of 13, 12, 1 and 6 rows (the largest divisor of H with at most 2048 pixels), 6 x 300
    pixels not a multiple of 256; x.c == y.c; an all-negative frame (max|y| is the largest |x|), a
    frame of zeros (its slot stays 0), a mixed frame. NCHW frames into the interior of a wider
    NHWC buffer; yc = 4 takes the one-store-per-pixel kernel."""
    x = nrm(3, xc, H, W, seed=9000 + H + W)
    x[0] = -x[0].abs() - 0.5
    x[1] = 0.0
    sw = yc
    sh = (W + 8) * sw
    y = Guarded((3, H, W, yc), ((H + 6) * sh, sh, sw, 1), 3 * sh + 4 * sw)
    ya = Guarded((3,), fill=0.0)
    ops.copy_pad(in_nhwc(x, "nchw"), y.view, y_amax=ya.view)
    torch.cuda.synchronize()
    got = y.cpu()
    assert torch.equal(got[..., :xc], x.permute(0, 2, 3, 1))
    assert torch.equal(got[..., xc:], torch.zeros(3, H, W, yc - xc))
    assert torch.equal(ya.cpu(), x.abs().amax(dim=(1, 2, 3)))
    assert ya.cpu()[1].item() == 0.0 and ya.cpu()[0].item() >= 0.5
    assert y.untouched() and ya.untouched()


def ns_ref(x):
    r = x.double() - x.double().mean(dim=(2, 3), keepdim=True)
    return torch.sigmoid(r / (r.std(dim=(2, 3), keepdim=True) + 1e-6))


@pytest.mark.parametrize("B,C,H,W,yk", [(2, 3, 2, 1024, "dense"), (2, 3, 2, 1025, "dense"), (2, 4, 2, 1024, "nchw"),
                                        (1, 4, 2, 1025, "nchw"), (2, 2, 5, 7, "inner"), (2, 1, 3, 1100, "odd")])
def test_norm_sigmoid_carry_and_constant_channel(B, C, H, W, yk):
    """W = 1024 (the 1024-thread walk advances one whole row, no column carry), W = 1025 (a carry
    every step), C = 4 into an NCHW view. The last channel of frame 0 is constant: mean exact,
    std 0, sigmoid(0) = 0.5 bit for bit."""
    x = uni(B, C, H, W, seed=9100 + W + C, scale=3.0) + 0.7
    x[0, C - 1] = 0.5
    y = g_nhwc(B, H, W, C, yk)
    ops.norm_sigmoid(in_nhwc(x, "inner" if yk == "inner" else "dense"), y.view)
    torch.cuda.synchronize()
    got = to_nchw(y)
    assert torch.equal(got[0, C - 1], torch.full((H, W), 0.5))
    keep = torch.ones(B, C, dtype=torch.bool)
    keep[0, C - 1] = False
    torch.testing.assert_close(got[keep].double(), ns_ref(x)[keep], rtol=0, atol=2e-6)
    assert y.untouched()
