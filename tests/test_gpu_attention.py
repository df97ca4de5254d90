"""GPU: the softmax-family attention kernels (csrc/attention.hip) across every schedule, route and
magnitude they can meet, against plain fp64 torch on the CPU.

ViT attention (L = 192, D = 64, the only size the kernel takes):
  1. every heads-per-workgroup schedule of the whole-head kernel (hpw = 1, 2, 3, 4, 6, 12; the
     register prefetch of head h + 1 and the re-staging of the LDS planes only run at hpw > 1):
     bit-identical to the same frames at hpw = 1, fp64 on three frames, planes output;
  2. the streaming kernel routed to at small B through an operand whose q / k / v lie 2^28 floats
     apart (a frame extent >= 2^31 bytes): hpw 1, 2, 3, its planes output, adversarial rows for its
     three-chunk online softmax;
  3. |logit| up to ~2000 on both kernels, against a bound derived from the 3-term bf16 split and
     against a CPU emulation of that split.
PSA attention: both kernels on either side of the 64 KiB switch, non-square maps, dk / dh below
the streaming kernel's register widths, strided views, peaky rows.

Tolerances: 5e-5 abs against fp64 on O(1) data (the project's bar for the split-bf16 x3 products),
1e-4 between the two ViT kernels, 1e-5 for the fp32 VALU PSA kernels; the extreme cases use the
bounds written out at their tests.
"""
import math

import pytest
import torch

from prpe import ops
from prpe._lib import PrpeError
from test_gpu_ops import _decode_planes

pytestmark = pytest.mark.gpu
DEV = "cuda"
L, D = 192, 64
SCALE = D ** -0.5
WHICH = 1 << 28                                          # q -> k -> v distance of the sparse operand


def _g(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return (torch.rand(*shape, generator=_g(seed)) * 2 - 1) * scale


def dev_rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand(*shape, generator=g, device=DEV) * 2 - 1) * scale


def launch_hpw(B, H):
    """attention_launch's rule: the largest divisor of H that leaves >= 256 workgroups."""
    hpw = H
    while hpw > 1 and (B * H // hpw < 256 or H % hpw):
        hpw -= 1
    return hpw


def ref64(x):
    """x: [n, L, 3, H, D] (any float dtype, CPU) -> softmax(q k^T * scale) v as fp64 [n, L, H * D]."""
    n, _, _, H, _ = x.shape
    q, k, v = x.permute(2, 0, 3, 1, 4).double()
    att = torch.softmax(q @ k.transpose(-1, -2) * SCALE, -1)
    return (att @ v).transpose(1, 2).reshape(n, L, H * D)


def whole(qkv, B, H, planes=False):
    """Row-major [B * L, 3 * H * D] operand: the whole-head kernel."""
    out = torch.empty(B * L, H * D, device=DEV)
    if planes:
        return ops.attention_strided(qkv, (L * 3 * H * D, H * D, D, 3 * H * D), out, B, L, H, D, SCALE,
                                     out_planes=True)
    return ops.attention(qkv, out, B, L, H, D, SCALE)


def whole_hpw1(qkv, B, H):
    """The same frames in slices of at most 256 // H frames: every launch has hpw = 1."""
    step = 256 // H
    assert launch_hpw(step, H) == 1
    out = torch.empty(B * L, H * D, device=DEV)
    for f in range(0, B, step):
        n = min(step, B - f)
        ops.attention(qkv[f * L:(f + n) * L], out[f * L:(f + n) * L], n, L, H, D, SCALE)
    return out


def assert_planes_are_split_of(pl, v32):
    n = v32.shape[0]
    hi, lo = _decode_planes(pl.cpu().view(n, 1, 1, -1))
    v = v32.cpu().view(n, 1, 1, -1)
    assert torch.equal(hi, v.to(torch.bfloat16).float())
    assert torch.equal(lo, (v - hi).to(torch.bfloat16).float())


# ------------------------------------------------------------------ 1. heads-per-workgroup schedules
SCHEDULES = [
    (43, 12, 2),      # hpw 2
    (64, 12, 3),      # hpw 3
    (86, 12, 4),      # hpw 4
    (128, 12, 6),     # hpw 6
    (256, 12, 12),    # hpw 12
    (64, 8, 2),       # hpw 2
    (256, 2, 2),      # hpw 2: every head of a frame in one workgroup
    (300, 1, 1),      # hpw 1: one head
    (52, 5, 1),       # hpw 1: a prime H has no divisor that leaves 256 workgroups
]


@pytest.mark.parametrize("B,H,hpw", SCHEDULES)
def test_vit_attention_hpw_schedule_bit_identical_to_hpw1(B, H, hpw):
    """Heads >= 1 of a workgroup's group come from the register prefetch issued under the previous
    head's MFMAs and are staged into LDS planes the previous head has just read: the result must
    not depend on that (README: frames are bit-identical whatever the batch)."""
    assert launch_hpw(B, H) == hpw
    qkv = dev_rnd(B * L, 3 * H * D, seed=1000 + B + H, scale=2.0)
    a = whole(qkv, B, H)
    b = whole_hpw1(qkv, B, H)
    torch.cuda.synchronize()
    if not torch.equal(a, b):
        bad = (a != b).view(B, L, H, D).any(3).any(1).nonzero()
        raise AssertionError(f"hpw {hpw} differs from hpw 1 at (frame, head) {bad[:8].tolist()} ... "
                             f"{bad.shape[0]} of {B * H}, max|d| {float((a - b).abs().max()):.3e}")


@pytest.mark.parametrize("B,H,hpw", SCHEDULES)
def test_vit_attention_hpw_schedule_fp64(B, H, hpw):
    assert launch_hpw(B, H) == hpw
    qkv = dev_rnd(B * L, 3 * H * D, seed=1000 + B + H, scale=2.0)
    out = whole(qkv, B, H).view(B, L, H * D)
    torch.cuda.synchronize()
    fr = [0, B // 2, B - 1]
    ref = ref64(qkv.view(B, L, 3, H, D)[fr].cpu())
    torch.testing.assert_close(out[fr].cpu(), ref.float(), rtol=0, atol=5e-5)


@pytest.mark.parametrize("B,H,hpw", [(64, 12, 3), (256, 12, 12)])
def test_vit_attention_hpw_schedule_planes_output(B, H, hpw):
    """out_planes at hpw > 1 == the (hi, lo) split of the hpw = 1 fp32 output, bit for bit."""
    assert launch_hpw(B, H) == hpw
    qkv = dev_rnd(B * L, 3 * H * D, seed=1000 + B + H, scale=2.0)
    pl = whole(qkv, B, H, planes=True)
    v32 = whole_hpw1(qkv, B, H)
    torch.cuda.synchronize()
    assert_planes_are_split_of(pl, v32)


# ------------------------------------------------------------------ 2. the streaming kernel, small B
def sparse_strides(H):
    return (L * H * D, WHICH, D, H * D)


def to_sparse(x):
    """x: CPU or device [B, L, 3, H, D] -> (buffer, strides) with q, k and v 2^28 floats apart in
    one otherwise unwritten buffer, so the frame extent is beyond a 32-bit byte offset and
    attention_launch takes the streaming kernel."""
    B, _, _, H, _ = x.shape
    n = B * L * H * D
    assert n <= WHICH
    buf = torch.empty(2 * WHICH + n, device=DEV)
    for w in range(3):
        buf[w * WHICH:w * WHICH + n].view(B, L, H, D).copy_(x[:, :, w])
    st = sparse_strides(H)
    assert ((L - 1) * st[3] + 2 * st[1] + (H - 1) * st[2] + D) * 4 >= (1 << 31)
    return buf, st


def stream(x, planes=False):
    B, _, _, H, _ = x.shape
    buf, st = to_sparse(x)
    out = ops.attention_strided(buf, st, torch.empty(B * L, H * D, device=DEV), B, L, H, D, SCALE,
                                out_planes=planes)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,hpw", [(2, 1), (43, 2), (64, 3)])
def test_vit_attention_streaming_kernel_small_batch(B, hpw):
    H = 12
    assert launch_hpw(B, H) == hpw
    x = dev_rnd(B, L, 3, H, D, seed=2000 + B, scale=2.0)
    s = stream(x).view(B, L, H * D).cpu()
    w = whole(x.view(B * L, 3 * H * D), B, H).view(B, L, H * D).cpu()
    xc = x.cpu()
    for f in range(0, B, 16):
        torch.testing.assert_close(s[f:f + 16], ref64(xc[f:f + 16]).float(), rtol=0, atol=5e-5)
    torch.testing.assert_close(s, w, rtol=0, atol=1e-4)       # two kernels, each within 5e-5 of fp64


@pytest.mark.parametrize("B", [2, 64])
def test_vit_attention_streaming_kernel_planes_output(B):
    H = 12
    x = dev_rnd(B, L, 3, H, D, seed=2100 + B, scale=2.0)
    assert_planes_are_split_of(stream(x, planes=True), stream(x))


def test_vit_attention_streaming_kernel_online_softmax_rescale():
    """The streaming kernel walks a head's keys in three chunks of 64 with a running max / sum and a
    rescale of O: dominant keys in chunk 0, 1 and 2 (the rescale factor is tiny when the dominant key
    comes late and the later chunks' weights are tiny when it comes first), a row maximum that rises
    in every chunk, uniform rows (a zero query; a head of identical keys)."""
    B, H = 1, 12
    x = rnd(B, L, 3, H, D, seed=2200)
    for q, key, c in ((5, 30, 4.0), (40, 3, 8.0),            # chunk 0
                      (100, 65, 4.0), (17, 127, 8.0),        # chunk 1
                      (60, 170, 4.0), (191, 191, 8.0)):      # chunk 2
        x[0, key, 1, 2] = c * x[0, q, 0, 2]                  # head 2: logit c |q|^2 / 8 ~ 2.7 c
    for key, c in ((10, 1.0), (80, 2.0), (150, 4.0)):        # head 3, query 33: max 2.7, 5.3, 10.7
        x[0, key, 1, 3] = c * x[0, 33, 0, 3]
    x[0, 7, 0, 5] = 0.0                                      # head 5, query 7: all logits 0
    x[0, :, 1, 8] = x[0, 0, 1, 8].clone()                    # head 8: every key the same
    s = stream(x.to(DEV)).view(B, L, H * D).cpu()
    ref = ref64(x)
    torch.testing.assert_close(s, ref.float(), rtol=0, atol=5e-5)
    # uniform rows are the mean of v
    vm = x[0, :, 2].double().mean(0)                         # [H, D]
    torch.testing.assert_close(s[0, 7, 5 * D:6 * D].double(), vm[5], rtol=0, atol=5e-5)
    torch.testing.assert_close(s[0, :, 8 * D:9 * D].double(), vm[8].expand(L, D), rtol=0, atol=5e-5)
    w = whole(x.view(B * L, 3 * H * D).to(DEV), B, H).view(B, L, H * D).cpu()
    torch.testing.assert_close(s, w, rtol=0, atol=1e-4)


# ------------------------------------------------------------------ 3. softmax extremes
def split_bf16(t):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def emulate_split(x):
    """CPU fp32 emulation of the kernels' arithmetic: every operand as hi = RNE bf16(x),
    lo = RNE bf16(x - hi); three products lo*hi + hi*lo + hi*hi accumulated in fp32; q pre-scaled
    into base-2 units, exp2 of (s - max); P split the same way for P V."""
    q, k, v = x.permute(2, 0, 3, 1, 4).float()
    qh, ql = split_bf16(q * (SCALE * 1.44269504088896340736))
    kh, kl = (t.transpose(-1, -2) for t in split_bf16(k))
    vh, vl = split_bf16(v)
    s = ql @ kh + qh @ kl + qh @ kh
    p = torch.exp2(s - s.max(-1, keepdim=True)[0])
    ph, pl = split_bf16(p)
    o = (ph @ vl + pl @ vh + ph @ vh) / p.sum(-1, keepdim=True)
    n, H = o.shape[:2]
    return o.transpose(1, 2).reshape(n, L, H * D)


def extreme_case(amp):
    B, H = 2, 12
    x = rnd(B, L, 3, H, D, seed=3000 + amp, scale=2.0)
    x[:, :, :2] *= amp / 2.0                                 # q and k uniform +-amp, v +-2
    x[0, 50, 1, 1] = x[0, 20, 0, 1]                          # a key equal to a query: logit |q|^2 / 8
    x[1, 7, 0, 5] = 0.0                                      # a zero query
    x[1, :, 1, 9] = x[1, :, 1, 9].abs()                      # head 9 of frame 1: positive keys and
    x[1, 100, 0, 9] = -0.5 * amp                             # one negative query: logits ~ -2 amp^2
    return x


def split_bound(x):
    """bound_id = (2 max_j delta_ij + 2^-16 + 2^-20) sum_j p_ij |v_jd|, delta_ij = 2^-16 scale
    sum_d |q_id| |k_jd|: each operand is two bf16 planes, each of the three products is off by at
    most 2^-18 of |q| |k| (the dropped lo*lo term and the two lo roundings), so a logit is off by at
    most delta, a weight by exp(+-2 delta) (numerator and denominator); P V is split the same way
    (2^-16); the fp32 accumulation over 64 terms and the output rounding lie beneath 2^-20."""
    n, _, _, H, _ = x.shape
    q, k, v = x.permute(2, 0, 3, 1, 4).double()
    p = torch.softmax(q @ k.transpose(-1, -2) * SCALE, -1)
    delta = 2.0 ** -16 * SCALE * (q.abs() @ k.abs().transpose(-1, -2))
    bound = (2 * delta.max(-1, keepdim=True)[0] + 2.0 ** -16 + 2.0 ** -20) * (p @ v.abs())
    return (p @ v).transpose(1, 2).reshape(n, L, H * D), bound.transpose(1, 2).reshape(n, L, H * D)


@pytest.mark.parametrize("kernel", ["whole", "stream"])
@pytest.mark.parametrize("amp", [2, 12, 30])
def test_vit_attention_logit_extremes(amp, kernel):
    """max |logit| ~ 10 (amp 2), ~ 350 (amp 12) and ~ 2000 (amp 30): finite, inside the elementwise
    bound of the 3-term split (split_bound), and at most 4x the max error of the CPU emulation of
    the same split on the same inputs (emulate_split; 4 covers the MFMA accumulation order,
    v_exp_f32 and v_rcp_f32). 5e-5 cannot be the bar here: the emulation itself is ~3e-4 off at
    amp 12.

    Measured on the MI355X (max error; max of error / bound; max error / the emulation's max error):
      amp  2 (max |logit|   10)  whole-head 9.06e-06  0.030  1.00   streaming 9.32e-06  0.030  1.03
      amp 12 (max |logit|  391)  whole-head 8.06e-04  0.069  1.00   streaming 7.61e-04  0.076  0.94
      amp 30 (max |logit| 2540)  whole-head 3.85e-03  0.095  1.03   streaming 4.15e-03  0.051  1.11
    The emulation itself: 9.07e-06 / 8.08e-04 / 3.74e-03, at most 0.10 of the bound.
    """
    x = extreme_case(amp)
    B, _, _, H, _ = x.shape
    if kernel == "whole":
        out = whole(x.view(B * L, 3 * H * D).to(DEV), B, H)
        torch.cuda.synchronize()
    else:
        out = stream(x.to(DEV))
    out = out.view(B, L, H * D).cpu().double()
    ref, bound = split_bound(x)
    logit = (x[:, :, 0].transpose(1, 2).double() @ x[:, :, 1].permute(0, 2, 3, 1).double() * SCALE).abs().max()
    err = (out - ref).abs()
    emu = (emulate_split(x).double() - ref).abs()
    print(f"\namp {amp} {kernel}: max|logit| {float(logit):.0f}  max err {float(err.max()):.3e}  "
          f"err/bound {float((err / bound).max()):.4f}  emulation max err {float(emu.max()):.3e}  "
          f"emulation/bound {float((emu / bound).max()):.4f}  err/emulation {float(err.max() / emu.max()):.3f}")
    assert torch.isfinite(out).all()
    assert (emu <= bound).all()                              # the yardstick itself obeys the bound
    assert (err <= bound).all(), f"max err / bound = {float((err / bound).max()):.3f}"
    assert float(err.max()) <= 4 * float(emu.max())


# ------------------------------------------------------------------ 4. PSA attention
def psa_ref(qkv, nh, dk, dh):
    """qkv: CPU [B, nh * (2 dk + dh), h, w] -> (out, v) fp64 [B, nh * dh, h, w]."""
    B, _, h, w = qkv.shape
    t = qkv.reshape(B, nh, 2 * dk + dh, h * w).double()
    q, k, v = t.split([dk, dk, dh], dim=2)
    att = ((q.transpose(-2, -1) @ k) * dk ** -0.5).softmax(-1)
    return (v @ att.transpose(-2, -1)).reshape(B, nh * dh, h, w), v.reshape(B, nh * dh, h, w)


def psa_run(qkv, nh, dk, dh):
    B, _, h, w = qkv.shape
    out = torch.empty(B, h, w, nh * dh, device=DEV)
    vout = torch.empty(B, h, w, nh * dh, device=DEV)
    ops.psa_attention(qkv.permute(0, 2, 3, 1).contiguous().to(DEV), out, vout, nh, dk, dh, dk ** -0.5)
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu(), vout.permute(0, 3, 1, 2).cpu()


def psa_streams(h, w, nh):
    return nh * (h * w) ** 2 * 4 > 64 * 1024


@pytest.mark.parametrize("h,w,nh,dk,dh,streams", [
    (3, 7, 2, 32, 64, False),      # LDS kernel, non-square
    (9, 10, 2, 32, 64, False),     # L = 90: the largest map the LDS kernel takes (64,800 B of scores)
    (7, 13, 2, 32, 64, True),      # L = 91: the smallest map on the streaming kernel
    (8, 15, 2, 32, 64, True),      # streaming kernel, non-square
    (1, 257, 2, 32, 64, True),     # a second blockIdx.y with one live thread
    (20, 20, 1, 16, 32, True),     # the streaming kernel's d < dk / d < dh masks
    (20, 20, 3, 24, 48, True),
    (5, 5, 1, 40, 80, False),      # the LDS kernel has no dk / dh cap
])
def test_psa_attention_shapes(h, w, nh, dk, dh, streams):
    assert psa_streams(h, w, nh) == streams
    B = 3
    qkv = rnd(B, nh * (2 * dk + dh), h, w, seed=4000 + h * w + dk, scale=2.0)
    out, vout = psa_run(qkv, nh, dk, dh)
    ref, v = psa_ref(qkv, nh, dk, dh)
    torch.testing.assert_close(out, ref.float(), rtol=0, atol=1e-5)
    assert torch.equal(vout, v.float())


def test_psa_attention_streaming_kernel_rejects_wide_heads():
    """dk = 40, dh = 80 (fine at 5x5, above) is beyond the streaming kernel's 32 / 64 registers."""
    B, nh, dk, dh, hw = 3, 1, 40, 80, 20
    assert psa_streams(hw, hw, nh)
    qkv = rnd(B, hw, hw, nh * (2 * dk + dh), seed=4100).to(DEV)
    out = torch.empty(B, hw, hw, nh * dh, device=DEV)
    with pytest.raises(PrpeError):
        ops.psa_attention(qkv, out, None, nh, dk, dh, dk ** -0.5)
    with pytest.raises(PrpeError):                           # dh alone
        ops.psa_attention(qkv[..., :2 * 32 + dh], out, None, nh, 32, dh, dk ** -0.5)


@pytest.mark.parametrize("h,w", [(3, 7), (8, 15)])
def test_psa_attention_strided_views(h, w):
    """qkv, out and vout as channel slices of wider buffers (pixel stride != channels): both
    kernels address through the view's strides and leave the bytes outside the slices alone."""
    B, nh, dk, dh = 3, 2, 32, 64
    c = nh * (2 * dk + dh)
    qkv = rnd(B, c, h, w, seed=4200 + h, scale=2.0)
    wide = torch.full((B, h, w, c + 24), float("nan"), device=DEV)
    wide[..., 8:8 + c] = qkv.permute(0, 2, 3, 1).to(DEV)
    obuf = torch.full((B, h, w, nh * dh + 40), -7.0, device=DEV)
    vbuf = torch.full((B, h, w, nh * dh + 16), -9.0, device=DEV)
    out, vout = obuf[..., 32:32 + nh * dh], vbuf[..., 4:4 + nh * dh]
    ops.psa_attention(wide[..., 8:8 + c], out, vout, nh, dk, dh, dk ** -0.5)
    torch.cuda.synchronize()
    ref, v = psa_ref(qkv, nh, dk, dh)
    torch.testing.assert_close(out.permute(0, 3, 1, 2).cpu(), ref.float(), rtol=0, atol=1e-5)
    assert torch.equal(vout.permute(0, 3, 1, 2).cpu(), v.float())
    assert bool((obuf[..., :32] == -7.0).all()) and bool((obuf[..., 32 + nh * dh:] == -7.0).all())
    assert bool((vbuf[..., :4] == -9.0).all()) and bool((vbuf[..., 4 + nh * dh:] == -9.0).all())
    assert bool(wide[..., :8].isnan().all()) and bool(wide[..., 8 + c:].isnan().all())


@pytest.mark.parametrize("h,w", [(9, 10), (20, 20)])
def test_psa_attention_peaky_rows(h, w):
    """One dominant key per chosen query (k_j a multiple of q_i: a logit of 60, the others' |logit|
    below 6) in the first, a middle and the last key position, plus an all-zero query (uniform
    weights), on the LDS kernel (9x10) and on the streaming kernel (20x20: keys in chunks of 64, the
    row maximum in a first pass).

    bound = (2 dk 2^-24 scale max_j sum_d |q||k| + (L + 8) 2^-24) sum_j p |v|: a sequential fp32
    dot of dk terms for the logit (on numerator and denominator), a sequential fp32 sum of L weights
    and of L products, expf and the division within a few ulp.

    Measured on the MI355X: 9x10 max error 2.43e-06, at most 0.010 of the bound; 20x20 max error
    1.25e-05, at most 0.036 of the bound.
    """
    B, nh, dk, dh = 3, 2, 32, 64
    per, Lp = 2 * dk + dh, h * w
    qkv = rnd(B, nh * per, h, w, seed=4300 + h, scale=2.0)
    t = qkv.view(B, nh, per, Lp)
    for n, hd, i, j in ((0, 0, 3, 0), (0, 1, Lp - 1, Lp // 2), (1, 0, Lp // 2, Lp - 1), (2, 1, 0, 65), (2, 0, 70, 70)):
        qi = t[n, hd, :dk, i]
        t[n, hd, dk:2 * dk, j] = qi * (60.0 * dk ** 0.5 / float(qi @ qi))     # logit (i, j) = 60
    t[1, 1, :dk, 11] = 0.0
    out, vout = psa_run(qkv, nh, dk, dh)
    ref, v = psa_ref(qkv, nh, dk, dh)
    q, k, vv = t.double().split([dk, dk, dh], dim=2)
    scale = dk ** -0.5
    logit = (q.transpose(-2, -1) @ k) * scale
    top2 = logit.topk(2, -1)[0]
    gap = top2[..., 0] - top2[..., 1]
    assert float(gap[0, 0, 3]) > 50 and float(gap[2, 0, 70]) > 50
    p = logit.softmax(-1)                                                        # [B, nh, i, j]
    qk = (q.abs().transpose(-2, -1) @ k.abs()).max(-1)[0]                        # [B, nh, i]
    bound = (2 * dk * 2.0 ** -24 * scale * qk + (Lp + 8) * 2.0 ** -24).unsqueeze(2) * (vv.abs() @ p.transpose(-2, -1))
    bound = bound.reshape(B, nh * dh, h, w)
    err = (out.double() - ref).abs()
    print(f"\npsa peaky {h}x{w}: max err {float(err.max()):.3e}  err/bound {float((err / bound).max()):.4f}")
    assert torch.isfinite(out).all()
    assert (err <= bound).all(), f"max err / bound = {float((err / bound).max()):.3f}"
    assert torch.equal(vout, v.float())
