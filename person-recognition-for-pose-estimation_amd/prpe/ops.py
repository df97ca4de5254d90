"""Torch-tensor level wrappers over the C ABI (device buffers come from PyTorch-ROCm).

Tensors are float32 on the GPU with a *logical NHWC* shape [N, H, W, C] and arbitrary
strides (channel slices of concat buffers, NCHW inputs via ``permute``, broadcast
residuals with stride 0 ...); the source frames of ``frame_ingest`` / ``crop_resize_u8`` are uint8
[N, H, W, 3]. Every call launches on the current torch stream.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from ._lib import ACT, NV12, RES_NONE, AnnotateArgs, BneckDesc, ConvDesc, IngestSrc, PrpeError, StemDesc, View, check, lib
from .arch import VIT_IMG


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t) -> int | None:
    return None if t is None else _gpu(t).data_ptr()


def _gpu(*ts):
    """Every tensor handed to the library must live in device memory: a host pointer in a
    kernel is a GPU memory fault, so it is refused here, before the C ABI."""
    for t in ts:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError(f"prpe: expected a HIP device tensor, got {type(t).__name__} on "
                             f"{getattr(t, 'device', '?')}")
    return ts[0] if len(ts) == 1 else ts


def view(t: torch.Tensor | None) -> View:
    """prpe_view of a 4-D logical-NHWC tensor (or a null view for None)."""
    if t is None:
        return View()
    assert t.dim() == 4 and t.dtype == torch.float32 and t.is_cuda, (t.shape, t.dtype, t.device)
    n, h, w, c = t.shape
    sn, sh, sw, sc = t.stride()
    return View(t.data_ptr(), n, h, w, c, sn, sh, sw, sc)


def nhwc(t: torch.Tensor) -> torch.Tensor:
    """Logical NHWC view of an NCHW tensor (no copy)."""
    return t.permute(0, 2, 3, 1)


def _check_slots(what, n, *slots):
    """max|x| / max|y| slot arrays: contiguous float32 device tensors of at least n (frames)
    entries -- the kernels index them by frame, so a short array would be read or raised out of
    bounds on the device."""
    for a in slots:
        if a is not None and (not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or not a.is_cuda or
                              a.numel() < n or not a.is_contiguous()):
            raise ValueError(f"{what}: max|x| slots must be a contiguous float32 device [N >= {n}]")


def conv2d(x, pack, y, *, res=None, res_mode=RES_NONE, act=None, precision=0, tile=0, x_amax=None,
           y_amax=None, x2=None, x2_amax=None, x_planes=False, y_planes=False, w2=None, y2=None, w3=None,
           scale2=None, bias2=None, act2="none"):
    """y = EPI(conv(PRO(x))) with a ``ConvPack`` (see prpe.pack).

    precision 3 (split fp16) and 4 (one fp16 plane) need ``x_amax``: a [N] device tensor,
    x_amax[n] bounding max|x[n]| per frame (e.g. the ``y_amax`` its producer raised). ``y_amax``
    (any precision): [N] device tensor the kernel raises to max|y[n]| per frame (zero it first)."""
    d = ConvDesc()
    _gpu(pack.w_hi)
    _check_slots(f"prpe_conv2d[{pack.name}]", x.shape[0], x_amax, y_amax, x2_amax)
    if precision in (3, 4):
        h16, l16, s16 = pack.f16_planes()
        d.w_h16, d.w_l16, d.scale16 = h16.data_ptr(), l16.data_ptr(), s16.data_ptr()
        d.x_amax = _ptr(x_amax)
    d.y_amax = _ptr(y_amax)
    d.x_planes, d.y_planes = int(x_planes), int(y_planes)   # planes format, see prpe.h
    if w2 is not None:                 # epilogue 1x1 GEMM (w2 fp32 [n2][Co]) into y2, see prpe.h
        _gpu(w2, y2)
        n_mid = y2.shape[3] if w3 is None else w3.shape[1]
        if w2.dtype != torch.float32 or not w2.is_contiguous() or w2.shape != (n_mid, y.shape[3]):
            raise ValueError(f"prpe_conv2d[{pack.name}]: w2 must be contiguous float32 [n2, Co]")
        d.w2 = w2.data_ptr()
        d.y2 = view(y2)
        if w3 is not None:             # second stage: z1 = act2(scale2 (y' w2^T) + bias2), z = z1 w3^T
            for t, shp in ((w3, (y2.shape[3], n_mid)), (scale2, (n_mid,)), (bias2, (n_mid,))):
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape != shp):
                    raise ValueError(f"prpe_conv2d[{pack.name}]: w3 [n3, n2] / scale2, bias2 [n2] float32")
            d.w3, d.scale2, d.bias2 = w3.data_ptr(), _ptr(scale2), _ptr(bias2)
            d.act2, d.n2 = ACT[act2], n_mid
    if x2 is not None:                 # second 1x1 input, see prpe.h (dual input)
        d.x2 = view(x2)
        d.x2_amax = _ptr(x2_amax)
    d.x = view(x)
    d.y = view(y)
    d.res = view(res)
    d.kh, d.kw, d.stride, d.pad = pack.kh, pack.kw, pack.stride, pack.pad
    d.w_hi, d.w_lo, d.w_lo2 = pack.w_hi.data_ptr(), pack.w_lo.data_ptr(), pack.w_lo2.data_ptr()
    d.k_pad, d.co_pad = pack.k_pad, pack.co_pad
    d.scale, d.bias, d.slope = _ptr(pack.scale), _ptr(pack.bias), _ptr(pack.slope)
    d.in_scale, d.in_bias = _ptr(pack.in_scale), _ptr(pack.in_bias)
    d.act = ACT[act if act is not None else pack.act]
    d.res_mode = res_mode
    d.precision = precision
    d.tile = tile
    d.k_order = pack.k_order
    # caller-owned scratch (the split-K partial sums; 0 bytes on every other path), from the
    # caching allocator on the current stream, so concurrent streams never share one
    nbytes = lib().prpe_conv2d_workspace_bytes(C.byref(d))
    if nbytes < 0:
        raise PrpeError(f"prpe_conv2d[{pack.name}]: descriptor rejected (status {nbytes})")
    ws = None
    if nbytes:
        ws = torch.empty((nbytes + 255) // 256 * 64, device=y.device, dtype=torch.float32)
        d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    check(lib().prpe_conv2d(C.byref(d), _stream()), f"prpe_conv2d[{pack.name}]")
    return y


def bottleneck(x, packs, y, x_amax, y_amax=None):
    """Fused identity-shortcut ResNet bottleneck at precision 3 (prpe_bottleneck, include/prpe.h):
    y = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + x); ``packs`` = the three
    ConvPacks (BN folded, conv2 chunk-major), x_amax [N] per-frame max|x|, y_amax [N] raised."""
    _gpu(x, y, x_amax)
    if x_amax is None:
        raise ValueError("prpe_bottleneck: x_amax (per-frame max|x| of the block input) is required")
    _check_slots("prpe_bottleneck", x.shape[0], x_amax, y_amax)
    d = BneckDesc()
    d.x, d.y = view(x), view(y)
    d.x_amax, d.y_amax = x_amax.data_ptr(), _ptr(y_amax)
    d.mid = packs[0].co
    keep = []
    for i, pk in enumerate(packs):
        h16, l16, s16 = pk.f16_planes()
        b = pk.bias if pk.bias is not None else torch.zeros(pk.co, device=x.device)
        keep.append(b)
        d.w_h16[i], d.w_l16[i], d.scale16[i], d.bias[i] = h16.data_ptr(), l16.data_ptr(), s16.data_ptr(), b.data_ptr()
        d.k_pad[i] = pk.k_pad
    check(lib().prpe_bottleneck(C.byref(d), _stream()), "prpe_bottleneck")
    return y


def stem_maxpool(buf, h, w, x_amax, pack, y, y_amax=None):
    """ResNet-50 stem conv (7x7/2, BN, ReLU) + max-pool 3x3/2 in one launch (prpe_stem_maxpool,
    include/prpe.h). ``buf``: the zero-bordered NHWC4 frames [N, h+6, w+8, 4] (Engine.stem's
    buffer, image at rows / columns 3..); ``pack``: the stem's chunked precision-3 ConvPack
    (k_pad 224); y [N, h/4, w/4, 64]."""
    _gpu(buf, y, x_amax)
    if not buf.is_contiguous() or buf.dim() != 4 or buf.shape[3] != 4:
        raise PrpeError("stem_maxpool: buf must be a contiguous [N, H+6, W+8, 4] buffer")
    if x_amax is None:
        raise ValueError("prpe_stem_maxpool: x_amax (per-frame max|x| of the frames) is required")
    _check_slots("prpe_stem_maxpool", buf.shape[0], x_amax, y_amax)
    d = StemDesc()
    d.x, d.xsn, d.xsh = buf.data_ptr(), buf.stride(0), buf.stride(1)
    d.n, d.h, d.w = buf.shape[0], h, w
    d.x_amax = x_amax.data_ptr()
    h16, l16, s16 = pack.f16_planes()
    b = pack.bias if pack.bias is not None else torch.zeros(pack.co, device=buf.device)
    d.w_h16, d.w_l16, d.k_pad, d.scale16, d.bias = h16.data_ptr(), l16.data_ptr(), pack.k_pad, s16.data_ptr(), b.data_ptr()
    d.y = view(y)
    d.y_amax = _ptr(y_amax)
    check(lib().prpe_stem_maxpool(C.byref(d), _stream()), "prpe_stem_maxpool")
    return y


def upconv3x3(z, y, align_corners, scale=None, bias=None, slope=None, act="none", separable=False,
              y_planes=False, y_amax=None):
    """Fused one-pass kernel by default; ``separable=True`` runs the two-pass workspace form.
    ``y_amax`` ([N] device, zeroed): raised to max|y[n]| per frame (one-pass kernels only)."""
    _check_slots("prpe_upconv3x3", y.shape[0], y_amax)
    zv, yv = view(z), view(y)
    ws, nbytes = None, 0
    if separable:
        nbytes = lib().prpe_upconv3x3_workspace_bytes(C.byref(zv), C.byref(yv))
        ws = torch.empty((nbytes + 3) // 4, device=z.device, dtype=torch.float32)
    check(lib().prpe_upconv3x3(C.byref(zv), C.byref(yv), 1 if align_corners else 0, _ptr(scale), _ptr(bias),
                               _ptr(slope), ACT[act], int(y_planes), _ptr(y_amax), _ptr(ws), nbytes, _stream()),
          "prpe_upconv3x3")
    return y


def dwconv(x, y, w, k, stride, pad, scale, bias, act="none", res=None):
    check(lib().prpe_dwconv(C.byref(view(x)), C.byref(view(y)), C.byref(view(res)), _ptr(w), k, stride, pad,
                            _ptr(scale), _ptr(bias), ACT[act], _stream()), "prpe_dwconv")
    return y


def maxpool(x, y, k, stride, pad):
    check(lib().prpe_maxpool(C.byref(view(x)), C.byref(view(y)), k, stride, pad, _stream()), "prpe_maxpool")
    return y


def copy_pad(x, y, flip_w=False, y_amax=None):
    """y = x zero-padded in C; ``flip_w`` reads x mirrored along W (a negative-stride view,
    so the flip-test pass needs no flipped copy of the frames); ``y_amax`` ([N] device tensor,
    zeroed) is raised to max|y[n]| per frame."""
    xv = view(x)
    if flip_w:
        xv.ptr = x.data_ptr() + (x.shape[2] - 1) * x.stride(2) * x.element_size()
        xv.sw = -x.stride(2)
    check(lib().prpe_copy_pad(C.byref(xv), C.byref(view(y)), _ptr(y_amax), _stream()), "prpe_copy_pad")
    return y


def upsample_nearest2x(x, y):
    check(lib().prpe_upsample_nearest2x(C.byref(view(x)), C.byref(view(y)), _stream()), "prpe_upsample_nearest2x")
    return y


def norm_sigmoid(x, y):
    check(lib().prpe_norm_sigmoid(C.byref(view(x)), C.byref(view(y)), _stream()), "prpe_norm_sigmoid")
    return y


def layernorm(x2d, y2d, gamma, beta, eps=1e-12, relu=False, planes=False):
    """planes: write y2d in the planes format (prpe.h) for a precision-0 GEMM consumer."""
    _gpu(x2d, y2d, gamma, beta)
    rows, c = x2d.shape
    check(lib().prpe_layernorm(x2d.data_ptr(), x2d.stride(0), y2d.data_ptr(), y2d.stride(0), rows, c,
                               gamma.data_ptr(), beta.data_ptr(), eps, (1 if relu else 0) | (2 if planes else 0),
                               _stream()), "prpe_layernorm")
    return y2d


def attention(qkv, out, B, L, H, D, scale):
    _gpu(qkv, out)
    check(lib().prpe_attention(qkv.data_ptr(), out.data_ptr(), B, L, H, D, scale, _stream()), "prpe_attention")
    return out


def attention_strided(qkv, strides, out, B, L, H, D, scale, out_planes=False):
    """qkv: tensor holding q/k/v at element strides (frame, which, head, token), e.g. a
    head-major [B, 3, H, L, D] buffer: (3*H*L*D, H*L*D, L*D, D); the row-major [B*L, 3*H*D]
    operand of prpe_attention is (L*3*H*D, H*D, D, 3*H*D). out_planes: write out in the planes
    format (prpe.h) for a precision-0 GEMM consumer."""
    _gpu(qkv, out)
    sf, sw, sh, st = (int(v) for v in strides)
    check(lib().prpe_attention_strided(qkv.data_ptr(), sf, sw, sh, st, out.data_ptr(), B, L, H, D, scale,
                                       1 if out_planes else 0, _stream()), "prpe_attention_strided")
    return out


def psa_attention(qkv, out, vout, nh, dk, dh, scale):
    check(lib().prpe_psa_attention(C.byref(view(qkv)), C.byref(view(out)), C.byref(view(vout)), nh, dk, dh, scale,
                                   _stream()), "prpe_psa_attention")
    return out


def dfl_decode(head, out, nc, level_hw, strides):
    _gpu(head, out)
    B = head.shape[0]
    hw = (C.c_int32 * (2 * len(level_hw)))(*[v for hw_ in level_hw for v in hw_])
    st = (C.c_float * len(strides))(*[float(s) for s in strides])
    check(lib().prpe_dfl_decode(head.data_ptr(), out.data_ptr(), B, nc, len(level_hw), hw, st, _stream()),
          "prpe_dfl_decode")
    return out


def l2norm(x, emb, norm, eps=0.0):
    """emb = x / max(||x||, eps) per row, norm = ||x||. eps 0: torch.div(x, norm) (IR-50 output);
    eps 1e-12: F.normalize."""
    _gpu(x, emb, norm)
    rows, c = x.shape
    check(lib().prpe_l2norm(x.data_ptr(), emb.data_ptr(), norm.data_ptr(), rows, c, float(eps), _stream()),
          "prpe_l2norm")
    return emb, norm


def nms(pred, layout, conf=0.001, iou=0.65, max_nms=30000, max_det=300):
    """Batched device NMS -> (out [B,max_det,6], count [B] int32). layout 0: [B,4+nc,N]; 1: [B,N,4+nc]."""
    pred = _gpu(pred).contiguous()
    B = pred.shape[0]
    if layout == 0:
        nc, N = pred.shape[1] - 4, pred.shape[2]
    else:
        N, nc = pred.shape[1], pred.shape[2] - 4
    out = torch.empty(B, max_det, 6, device=pred.device, dtype=torch.float32)
    cnt = torch.empty(B, device=pred.device, dtype=torch.int32)
    # N*nc above the kernel's LDS key capacity: keys + a radix sort per image in a global workspace
    nbytes = lib().prpe_nms_workspace_bytes(B, N, nc, max_nms)
    if nbytes < 0:
        raise RuntimeError("prpe_nms_workspace_bytes failed")
    ws = torch.empty((nbytes + 7) // 8, device=pred.device, dtype=torch.int64) if nbytes else None
    check(lib().prpe_nms(pred.data_ptr(), B, N, nc, layout, conf, iou, max_nms, max_det, out.data_ptr(),
                         cnt.data_ptr(), _ptr(ws), nbytes, _stream()), "prpe_nms")
    return out, cnt


def softargmax(heat, boxes=None, want_argmax=False):
    heat = _gpu(heat).contiguous()
    B, K, H, W = heat.shape
    coords = torch.empty(B, K, 2, device=heat.device, dtype=torch.float32)
    scores = torch.empty(B, K, device=heat.device, dtype=torch.float32)
    am = torch.empty(B, K, device=heat.device, dtype=torch.int32) if want_argmax else None
    bx = boxes.contiguous().float() if boxes is not None else None
    check(lib().prpe_softargmax(heat.data_ptr(), B, K, H, W, _ptr(bx), coords.data_ptr(), scores.data_ptr(),
                                _ptr(am), _stream()), "prpe_softargmax")
    return (coords, scores, am) if want_argmax else (coords, scores)


def flip_average(heat, heat_flipped, partner, mode=0):
    """Pose flip test: (heat + flipback(heat_flipped)) * 0.5 (pose_estimation/module.py:470-484)."""
    heat, heat_flipped = (t.contiguous() for t in _gpu(heat, heat_flipped))
    B, K, H, W = heat.shape
    out = torch.empty_like(heat)
    pa = (C.c_int32 * K)(*[int(v) for v in partner])
    check(lib().prpe_flip_average(heat.data_ptr(), heat_flipped.data_ptr(), out.data_ptr(), B, K, H, W, pa, mode,
                                  _stream()), "prpe_flip_average")
    return out


def ce_argmax(logits, labels=None):
    """Per-row argmax (+ cross-entropy and the [mean loss, acc] summary when labels given)."""
    _gpu(logits)
    B, Cn = logits.shape
    assert logits.stride(1) == 1
    amax = torch.empty(B, device=logits.device, dtype=torch.int32)
    loss = summary = None
    if labels is not None:
        labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        loss = torch.empty(B, device=logits.device, dtype=torch.float32)
        summary = torch.empty(2, device=logits.device, dtype=torch.float32)
    check(lib().prpe_ce_argmax(logits.data_ptr(), logits.stride(0), B, Cn, _ptr(labels), _ptr(loss), amax.data_ptr(),
                               _ptr(summary), _stream()), "prpe_ce_argmax")
    return loss, amax, summary


def det_metrics_update(dets, counts, gt_boxes, gt_batch, counters, records):
    """Append one batch to the device DetectionMetrics state (see include/prpe.h)."""
    _gpu(dets, counts, counters, records)
    B, max_det, six = dets.shape
    assert six == 6 and dets.is_contiguous() and counts.dtype == torch.int32
    gt = gt_boxes.to(device=dets.device, dtype=torch.float32).contiguous().view(-1, 4)
    gb = gt_batch.to(device=dets.device, dtype=torch.int64).contiguous().view(-1)
    nbytes = lib().prpe_det_metrics_update_workspace_bytes(B)
    ws = torch.empty(max(1, (nbytes + 3) // 4), device=dets.device, dtype=torch.float32)
    check(lib().prpe_det_metrics_update(dets.data_ptr(), counts.contiguous().data_ptr(), B, max_det, gt.data_ptr(),
                                        gb.data_ptr(), gt.shape[0], counters.data_ptr(), records.data_ptr(),
                                        records.shape[0], ws.data_ptr(), nbytes, _stream()), "prpe_det_metrics_update")


def det_metrics_compute(counters, records, n, thresholds):
    """(precision, recall, f1, mAP50, mAP75, mAP) as a float64 device tensor [6]."""
    _gpu(counters, records)
    nbytes = lib().prpe_det_metrics_compute_workspace_bytes(n)
    ws = torch.empty((nbytes + 3) // 4, device=counters.device, dtype=torch.float32)
    out = torch.empty(6, device=counters.device, dtype=torch.float64)
    thr = (C.c_float * len(thresholds))(*[float(t) for t in thresholds])
    check(lib().prpe_det_metrics_compute(counters.data_ptr(), records.data_ptr(), n, C.cast(thr, C.c_void_p),
                                         out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "prpe_det_metrics_compute")
    return out


def det_eval_loss(boxes, scores, gt_boxes, gt_batch, gt_classes=None):
    """Detection eval loss (see include/prpe.h): boxes [B,4,N], scores [B,C,N] (any strides).
    Returns (loss [1], per_image [B,4] = (loss_b, box, cls, bg))."""
    _gpu(boxes, scores)
    B, four, N = boxes.shape
    Cn = scores.shape[1]
    assert four == 4 and scores.shape[0] == B and scores.shape[2] == N
    dev = boxes.device
    gt = gt_boxes.to(device=dev, dtype=torch.float32).contiguous().view(-1, 4)
    gb = gt_batch.to(device=dev, dtype=torch.int64).contiguous().view(-1)
    gc = None if gt_classes is None else gt_classes.to(device=dev, dtype=torch.int64).contiguous().view(-1)
    bs = (C.c_int64 * 3)(*boxes.stride())
    ss = (C.c_int64 * 3)(*scores.stride())
    per = torch.empty(B, 4, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    check(lib().prpe_det_eval_loss(boxes.data_ptr(), C.cast(bs, C.c_void_p), scores.data_ptr(), C.cast(ss, C.c_void_p),
                                   B, Cn, N, gt.data_ptr(), gb.data_ptr(), _ptr(gc), gt.shape[0], per.data_ptr(),
                                   loss.data_ptr(), _stream()), "prpe_det_eval_loss")
    return loss, per


def pose_eval_loss(heat, keypoints, kp_weights, *, heat_flipped=None, partner=None, mode=0, areas=None, boxes=None,
                   sigma=2.0, topk=8, avg_out=None, want_avg=False, want_argmax=False, want_target=False):
    """Fused pose validation step after the model (see include/prpe.h): heat [B,K,H,W] (+ the
    flipped pass' heat_flipped, averaged in registers), keypoints [B,N,K,3], areas [B,N] / boxes
    [B,N,4] optional, kp_weights host floats [K]. Returns a dict: loss [1], per_kp [B,K], coords
    [B,K,2], scores [B,K], and on request avg, argmax, target + weights."""
    heat, keypoints = _gpu(heat, keypoints)
    heat = heat.contiguous()
    assert heat.dtype == torch.float32, heat.dtype
    B, K, H, W = heat.shape
    dev = heat.device
    kp = keypoints.to(torch.float32).contiguous()
    assert kp.dim() == 4 and kp.shape[0] == B and kp.shape[2] == K and kp.shape[3] == 3, kp.shape
    N = kp.shape[1]
    if heat_flipped is not None:
        heat_flipped = _gpu(heat_flipped).contiguous()
        assert heat_flipped.shape == heat.shape and heat_flipped.dtype == torch.float32, heat_flipped.dtype
        if want_avg and avg_out is None:
            avg_out = torch.empty_like(heat)
    if avg_out is not None:
        assert avg_out.shape == heat.shape and avg_out.is_contiguous() and avg_out.dtype == torch.float32
    ar = None if areas is None else _gpu(areas).to(torch.float32).contiguous()
    bx = None if boxes is None else _gpu(boxes).to(torch.float32).contiguous()
    assert ar is None or tuple(ar.shape) == (B, N)
    assert bx is None or tuple(bx.shape) == (B, N, 4)
    if len(kp_weights) != K:
        raise ValueError(f"pose_eval_loss: {len(kp_weights)} keypoint weights for K = {K}")
    kw = (C.c_float * K)(*[float(v) for v in kp_weights])
    pa = None if partner is None else (C.c_int32 * K)(*[int(v) for v in partner])
    out = {"loss": torch.empty(1, device=dev), "per_kp": torch.empty(B, K, device=dev),
           "coords": torch.empty(B, K, 2, device=dev), "scores": torch.empty(B, K, device=dev)}
    if avg_out is not None:
        out["avg"] = avg_out
    if want_argmax:
        out["argmax"] = torch.empty(B, K, device=dev, dtype=torch.int32)
    if want_target:
        out["target"] = torch.empty_like(heat)
        out["weights"] = torch.empty(B, K, device=dev)
    check(lib().prpe_pose_eval_loss(heat.data_ptr(), _ptr(heat_flipped), pa, mode, _ptr(avg_out), B, K, H, W,
                                    kp.data_ptr(), _ptr(ar), _ptr(bx), N, float(sigma), kw, topk,
                                    out["per_kp"].data_ptr(), out["loss"].data_ptr(), out["coords"].data_ptr(),
                                    out["scores"].data_ptr(), _ptr(out.get("argmax")), _ptr(out.get("target")),
                                    _ptr(out.get("weights")), _stream()), "prpe_pose_eval_loss")
    return out


def pose_coco_records(coords, scores, boxes, areas, masks, is_crowd, keep, keypoint_thresh, slot_base, counter,
                      rec_kpts, rec_meta):
    """Append one batch's COCO keypoint records to the device state (see include/prpe.h):
    counter uint64 [1] (an int64 tensor), rec_kpts [cap,K,3], rec_meta [cap,8]. ``keep`` is a
    HOST sequence of B flags: it goes into the kernel arguments, so nothing is uploaded."""
    _gpu(coords, scores, boxes, areas, masks, is_crowd, counter, rec_kpts, rec_meta)
    B, K, two = coords.shape
    N = boxes.shape[1]
    assert two == 2 and coords.is_contiguous() and scores.is_contiguous() and tuple(scores.shape) == (B, K)
    assert coords.dtype == torch.float32 and scores.dtype == torch.float32
    bx = boxes.to(torch.float32).contiguous()
    ar = areas.to(torch.float32).contiguous()
    mk = masks.to(torch.uint8).contiguous()         # bool -> 0/1
    cr = is_crowd.to(torch.uint8).contiguous()
    if isinstance(keep, torch.Tensor):
        raise ValueError("pose_coco_records: keep is a host sequence of flags, not a tensor")
    kf = (C.c_uint8 * len(keep))(*[1 if v else 0 for v in keep])
    assert tuple(bx.shape) == (B, N, 4) and tuple(ar.shape) == (B, N) and tuple(mk.shape) == (B, N)
    assert tuple(cr.shape) == (B, N) and len(keep) == B
    cap = rec_kpts.shape[0]
    assert counter.dtype == torch.int64 and counter.numel() == 1
    assert rec_kpts.dtype == torch.float32 and rec_kpts.is_contiguous() and tuple(rec_kpts.shape) == (cap, K, 3)
    assert rec_meta.dtype == torch.float32 and rec_meta.is_contiguous() and tuple(rec_meta.shape) == (cap, 8)
    check(lib().prpe_pose_coco_records(coords.data_ptr(), scores.data_ptr(), bx.data_ptr(), ar.data_ptr(),
                                       mk.data_ptr(), cr.data_ptr(), kf, B, N, K, float(keypoint_thresh),
                                       int(slot_base), counter.data_ptr(), rec_kpts.data_ptr(), rec_meta.data_ptr(),
                                       cap, _stream()), "prpe_pose_coco_records")


# ------------------------------------------------------------------ COCO keypoint AP / AR (csrc/cocoeval.hip)
COCO_MAX_DETS, COCO_MAX_GT, COCO_IOU_THRS, COCO_REC_THRS, COCO_AREAS = 20, 64, 10, 101, 3
COCO_EMPTY_BIT = 63


def _host_doubles(what, name, v, n):
    v = [float(x) for x in v]
    if len(v) != n:
        raise ValueError(f"{what}: {name} needs {n} values, got {len(v)}")
    return (C.c_double * n)(*v)


def coco_kp_match(rec_kpts, rec_meta, counter, n_max, slot_to_img, gt_start, gt_kpts, gt_bbox, gt_area, gt_iscrowd,
                  gt_ignore, max_gt, sigmas, iou_thrs, area_rngs, *, want_oks=True, out=None):
    """COCOeval.evaluate() for keypoints on the device records (prpe_coco_kp_match, include/prpe.h).
    rec_kpts [cap,K,3] / rec_meta [cap,8] / counter int64 [1] (or None) as ``pose_coco_records``
    leaves them, ``n_max`` the host's bound on the records; slot_to_img int32 [slots]; the
    ground-truth table gt_start int32 [I+1], gt_kpts float64 [G,K,3], gt_bbox [G,4], gt_area [G],
    gt_iscrowd / gt_ignore uint8 [G], ``max_gt`` its largest image (host). Returns a dict of device
    tensors: dt_score float32 [I,20], dt_bits int64 [I,20], dt_rec int32 [I,20], npig int32 [I,3]
    and oks float64 [I,20,64]. ``out`` supplies them instead (all four, plus oks if wanted)."""
    what = "coco_kp_match"
    _check_dev(what, "gt_start", gt_start, torch.int32, min_numel=2)
    I = gt_start.numel() - 1
    dev = gt_start.device
    _check_dev(what, "rec_kpts", rec_kpts, torch.float32)
    if rec_kpts.dim() != 3 or rec_kpts.shape[2] != 3:
        raise ValueError(f"{what}: rec_kpts must be [cap, K, 3], got {list(rec_kpts.shape)}")
    cap, K = rec_kpts.shape[0], rec_kpts.shape[1]
    _check_dev(what, "rec_meta", rec_meta, torch.float32, (cap, 8))
    n_max = int(n_max)
    if n_max > cap:
        raise ValueError(f"{what}: n_max {n_max} exceeds the record arrays' capacity {cap}")
    if counter is not None:
        _check_dev(what, "counter", counter, torch.int64, (1,))
    _check_dev(what, "slot_to_img", slot_to_img, torch.int32)
    _check_dev(what, "gt_kpts", gt_kpts, torch.float64)
    if gt_kpts.dim() != 3 or tuple(gt_kpts.shape[1:]) != (K, 3):
        raise ValueError(f"{what}: gt_kpts must be [G, {K}, 3], got {list(gt_kpts.shape)}")
    G = gt_kpts.shape[0]
    _check_dev(what, "gt_bbox", gt_bbox, torch.float64, (G, 4))
    _check_dev(what, "gt_area", gt_area, torch.float64, (G,))
    _check_dev(what, "gt_iscrowd", gt_iscrowd, torch.uint8, (G,))
    _check_dev(what, "gt_ignore", gt_ignore, torch.uint8, (G,))
    sg = _host_doubles(what, "sigmas", sigmas, K)
    it = _host_doubles(what, "iou_thrs", iou_thrs, COCO_IOU_THRS)
    ar = _host_doubles(what, "area_rngs", [v for r in area_rngs for v in r], 2 * COCO_AREAS)
    if out is None:
        out = {"dt_score": torch.empty(I, COCO_MAX_DETS, device=dev),
               "dt_bits": torch.empty(I, COCO_MAX_DETS, device=dev, dtype=torch.int64),
               "dt_rec": torch.empty(I, COCO_MAX_DETS, device=dev, dtype=torch.int32),
               "npig": torch.empty(I, COCO_AREAS, device=dev, dtype=torch.int32)}
        if want_oks:
            out["oks"] = torch.empty(I, COCO_MAX_DETS, COCO_MAX_GT, device=dev, dtype=torch.float64)
    _check_dev(what, "dt_score", out["dt_score"], torch.float32, (I, COCO_MAX_DETS))
    _check_dev(what, "dt_bits", out["dt_bits"], torch.int64, (I, COCO_MAX_DETS))
    _check_dev(what, "dt_rec", out["dt_rec"], torch.int32, (I, COCO_MAX_DETS))
    _check_dev(what, "npig", out["npig"], torch.int32, (I, COCO_AREAS))
    if out.get("oks") is not None:
        _check_dev(what, "oks", out["oks"], torch.float64, (I, COCO_MAX_DETS, COCO_MAX_GT))
    nbytes = lib().prpe_coco_kp_match_workspace_bytes(I)
    ws = torch.empty(max(1, (nbytes + 3) // 4), device=dev, dtype=torch.int32)
    check(lib().prpe_coco_kp_match(rec_kpts.data_ptr(), rec_meta.data_ptr(), _ptr(counter), n_max,
                                   slot_to_img.data_ptr(), slot_to_img.numel(), gt_start.data_ptr(),
                                   gt_kpts.data_ptr(), gt_bbox.data_ptr(), gt_area.data_ptr(), gt_iscrowd.data_ptr(),
                                   gt_ignore.data_ptr(), I, G, int(max_gt), K, sg, it, ar, out["dt_score"].data_ptr(),
                                   out["dt_bits"].data_ptr(), out["dt_rec"].data_ptr(), out["npig"].data_ptr(),
                                   _ptr(out.get("oks")), ws.data_ptr(), nbytes, _stream()), "prpe_coco_kp_match")
    return out


def coco_kp_accumulate(dt_score, dt_bits, npig, rec_thrs, *, out=None):
    """COCOeval.accumulate() and summarize() for keypoints (prpe_coco_kp_accumulate) on
    ``coco_kp_match``'s tables. Returns device float64 tensors: precision [10,101,3], recall
    [10,3], stats [10] = AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl."""
    what = "coco_kp_accumulate"
    _check_dev(what, "dt_score", dt_score, torch.float32)
    if dt_score.dim() != 2 or dt_score.shape[0] < 1 or dt_score.shape[1] != COCO_MAX_DETS:
        raise ValueError(f"{what}: dt_score must be [I >= 1, {COCO_MAX_DETS}], got {list(dt_score.shape)}")
    I = dt_score.shape[0]
    dev = dt_score.device
    _check_dev(what, "dt_bits", dt_bits, torch.int64, (I, COCO_MAX_DETS))
    _check_dev(what, "npig", npig, torch.int32, (I, COCO_AREAS))
    rt = _host_doubles(what, "rec_thrs", rec_thrs, COCO_REC_THRS)
    if out is None:
        out = {"precision": torch.empty(COCO_IOU_THRS, COCO_REC_THRS, COCO_AREAS, device=dev, dtype=torch.float64),
               "recall": torch.empty(COCO_IOU_THRS, COCO_AREAS, device=dev, dtype=torch.float64),
               "stats": torch.empty(10, device=dev, dtype=torch.float64)}
    _check_dev(what, "precision", out["precision"], torch.float64, (COCO_IOU_THRS, COCO_REC_THRS, COCO_AREAS))
    _check_dev(what, "recall", out["recall"], torch.float64, (COCO_IOU_THRS, COCO_AREAS))
    _check_dev(what, "stats", out["stats"], torch.float64, (10,))
    nbytes = lib().prpe_coco_kp_accumulate_workspace_bytes(I)
    ws = torch.empty(max(1, (nbytes + 7) // 8), device=dev, dtype=torch.int64)
    check(lib().prpe_coco_kp_accumulate(dt_score.data_ptr(), dt_bits.data_ptr(), npig.data_ptr(), I, rt,
                                        out["precision"].data_ptr(), out["recall"].data_ptr(),
                                        out["stats"].data_ptr(), ws.data_ptr(), nbytes, _stream()),
          "prpe_coco_kp_accumulate")
    return out


# ------------------------------------------------------------------ top-down pose (csrc/topdown.hip)
CROP_META_COLS = 8
CROP_BORDER = 2                      # the patch conv's padding = the crop buffer's zero border


def _check_dev(what, name, t, dtype, shape=None, min_numel=None):
    """A contiguous device tensor of ``dtype`` and exactly ``shape`` (or at least ``min_numel``
    elements): the top-down kernels index these by slot / frame with no strides, so a short or
    strided one would be read or written out of bounds on the device. Raised here, on the host."""
    ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
    if ok and shape is not None:
        ok = tuple(t.shape) == tuple(shape)
    if ok and min_numel is not None:
        ok = t.numel() >= min_numel
    if not ok:
        want = f"{list(shape)}" if shape is not None else f"[>= {min_numel}]"
        got = (f"{type(t).__name__}" if not isinstance(t, torch.Tensor) else
               f"{t.dtype} {list(t.shape)} on {t.device}, contiguous={t.is_contiguous()}")
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} device tensor {want}, got {got}")


def crop_select(dets, counts, frame_hw, *, crop_meta, n_crops, status, score_thr=0.25, max_per_frame=8,
                min_size=4.0, box_scale=(1.0, 1.0), pad=1.25):
    """Padded NMS output -> the crop list (prpe_crop_select, include/prpe.h): dets [B, max_det, 6],
    counts [B] int32; ``frame_hw`` = (H, W) of the frames, ``box_scale`` = (x, y) detector units
    -> frame pixels. Fills crop_meta [max_crops, 8], n_crops [1] int32, status [1] int32 (bit 0:
    a frame's NMS overflowed, bit 1: crops dropped past max_crops). No host read."""
    what = "prpe_crop_select"
    if not (isinstance(dets, torch.Tensor) and dets.dim() == 3 and dets.shape[2] == 6):
        raise ValueError(f"{what}: dets must be [B, max_det, 6]")
    B, max_det, _ = dets.shape
    _check_dev(what, "dets", dets, torch.float32, (B, max_det, 6))
    _check_dev(what, "counts", counts, torch.int32, (B,))
    if not (isinstance(crop_meta, torch.Tensor) and crop_meta.dim() == 2):
        raise ValueError(f"{what}: crop_meta must be [max_crops, {CROP_META_COLS}]")
    max_crops = crop_meta.shape[0]
    _check_dev(what, "crop_meta", crop_meta, torch.float32, (max_crops, CROP_META_COLS))
    _check_dev(what, "n_crops", n_crops, torch.int32, (1,))
    _check_dev(what, "status", status, torch.int32, (1,))
    H, W = (int(v) for v in frame_hw)
    sx, sy = (float(v) for v in box_scale)
    if B < 1 or max_det < 1 or max_crops < 1 or max_per_frame < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: empty batch, crop list or frame")
    check(lib().prpe_crop_select(dets.data_ptr(), counts.data_ptr(), B, max_det, float(score_thr), int(max_per_frame),
                                 float(min_size), sx, sy, H, W, float(pad), max_crops, crop_meta.data_ptr(),
                                 n_crops.data_ptr(), status.data_ptr(), _stream()), what)
    return crop_meta, n_crops, status


def crop_resize(frames, crop_meta, n_crops, crops):
    """Resample the windows of ``crop_meta`` from ``frames`` ([B, 3, H, W] float32 device, any
    strides) into the interior of ``crops``, the zero-bordered NHWC4 buffer [max_crops, 260, 196, 4]
    (Engine.crop_pix4; prpe_crop_resize, include/prpe.h). Slots at or past n_crops are zeroed."""
    what = "prpe_crop_resize"
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.float32 and
            frames.dim() == 4 and frames.shape[1] == 3 and frames.numel() > 0):
        raise ValueError(f"{what}: frames must be a float32 device tensor [B, 3, H, W]")
    if not (isinstance(crop_meta, torch.Tensor) and crop_meta.dim() == 2):
        raise ValueError(f"{what}: crop_meta must be [max_crops, {CROP_META_COLS}]")
    max_crops = crop_meta.shape[0]
    shape =(max_crops, VIT_IMG[0] + 2 * CROP_BORDER, VIT_IMG[1] + 2 * CROP_BORDER, 4)
    _check_dev(what, "crop_meta", crop_meta, torch.float32, (max_crops, CROP_META_COLS))
    _check_dev(what, "n_crops", n_crops, torch.int32, (1,))
    _check_dev(what, "crops", crops, torch.float32, shape)
    if max_crops < 1 or crops.data_ptr() % 16:
        raise ValueError(f"{what}: crops must hold at least one slot and be 16-byte aligned")
    check(lib().prpe_crop_resize(C.byref(view(nhwc(frames))), crop_meta.data_ptr(), n_crops.data_ptr(), max_crops,
                                 crops.data_ptr(), _stream()), what)
    return crops


def crop_keypoints(coords, scores, crop_meta, n_crops, kpts):
    """Soft-argmax output of the first n slots (coords [n, K, 2] in [0,1] of the crop, scores
    [n, K]) -> kpts [max_crops, K, 3] = (x, y in frame pixels, score); slots at or past
    min(n_crops, n) are zeroed (prpe_crop_keypoints, include/prpe.h)."""
    what = "prpe_crop_keypoints"
    if not (isinstance(coords, torch.Tensor) and coords.dim() == 3 and coords.shape[2] == 2):
        raise ValueError(f"{what}: coords must be [n, K, 2]")
    n, K, _ = coords.shape
    if not (isinstance(crop_meta, torch.Tensor) and crop_meta.dim() == 2):
        raise ValueError(f"{what}: crop_meta must be [max_crops, {CROP_META_COLS}]")
    max_crops = crop_meta.shape[0]
    _check_dev(what, "coords", coords, torch.float32, (n, K, 2))
    _check_dev(what, "scores", scores, torch.float32, (n, K))
    _check_dev(what, "crop_meta", crop_meta, torch.float32, (max_crops, CROP_META_COLS))
    _check_dev(what, "n_crops", n_crops, torch.int32, (1,))
    _check_dev(what, "kpts", kpts, torch.float32, (max_crops, K, 3))
    if n < 1 or K < 1 or n > max_crops:
        raise ValueError(f"{what}: {n} crops of keypoints for a list of {max_crops} slots")
    check(lib().prpe_crop_keypoints(coords.data_ptr(), scores.data_ptr(), n, K, crop_meta.data_ptr(),
                                    n_crops.data_ptr(), max_crops, kpts.data_ptr(), _stream()), what)
    return kpts


# ------------------------------------------------------------------ uint8 frames in (csrc/ingest.hip)
def _u8_frames(what, frames):
    """prpe_view_u8 of source frames: a uint8 device tensor with the logical shape [B, Hs, Ws, 3]
    and any strides (an HWC batch, NCHW through ``permute(0, 2, 3, 1)``, a slice). Dtype, channel
    count and device are checked here, before the C ABI."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise ValueError(f"{what}: frames must be a uint8 tensor, got "
                         f"{getattr(frames, 'dtype', type(frames).__name__)}")
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError(f"{what}: frames must be [B, Hs, Ws, 3] (3 channels last; permute NCHW frames), got "
                         f"{list(frames.shape)}")
    if not frames.is_cuda:
        raise ValueError(f"{what}: frames must be a HIP device tensor, got one on {frames.device}")
    n, h, w, c = frames.shape
    return View(frames.data_ptr(), n, h, w, c, *frames.stride())


def _f3(what, name, v):
    v = [float(x) for x in v]
    if len(v) != 3:
        raise ValueError(f"{what}: {name} must hold 3 floats (one per output channel)")
    return (C.c_float * 3)(*v)


def frame_ingest(frames, y, region, a, b, fill=(0.0, 0.0, 0.0), swap_rb=False, y_amax=None):
    """uint8 frames [B, Hs, Ws, 3] (any strides) -> ``y``, the interior [B, H, W, 4] of a
    zero-bordered NHWC4 buffer (Engine.stem's): bilinear resize into ``region`` = (top, left, nh,
    nw), ``fill`` (raw 0..255 units) outside it, then raw * a[c] + b[c]; channel 3 = 0
    (prpe_frame_ingest, include/prpe.h). ``a``, ``b``, ``fill``: 3 host floats each. ``swap_rb``:
    the source is BGR. ``y_amax`` ([B] device, zeroed): raised to max|y[n]| per frame."""
    what = "prpe_frame_ingest"
    fv = _u8_frames(what, frames)
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 4):
        raise ValueError(f"{what}: y must be a float32 device tensor [B, H, W, 4]")
    if y.shape[0] != frames.shape[0] or y.shape[3] != 4 or y.stride(3) != 1 or y.data_ptr() % 16 or \
            any(s % 4 for s in y.stride()[:3]):
        raise ValueError(f"{what}: y must be [{frames.shape[0]}, H, W, 4] with 4 contiguous, 16-byte aligned "
                         f"channels, got {list(y.shape)} strides {list(y.stride())}")
    top, left, nh, nw = (int(v) for v in region)
    if nh < 1 or nw < 1 or top < 0 or left < 0 or top + nh > y.shape[1] or left + nw > y.shape[2]:
        raise ValueError(f"{what}: region {(top, left, nh, nw)} is empty or not inside {list(y.shape[1:3])}")
    _check_slots(what, frames.shape[0], y_amax)
    check(lib().prpe_frame_ingest(C.byref(fv), C.byref(view(y)), top, left, nh, nw, _f3(what, "a", a),
                                  _f3(what, "b", b), _f3(what, "fill", fill), int(bool(swap_rb)), _ptr(y_amax),
                                  _stream()), what)
    return y


INGEST_MAX_SCALE = 32      # prpe_frame_ingest_multi, filter 1: the largest downscale per axis


def frame_list(frames):
    """The frames of a batch as a list: a 4-D tensor is taken as its frames, a sequence as it is."""
    if isinstance(frames, torch.Tensor):
        return list(frames.unbind(0)) if frames.dim() == 4 else [frames]
    return list(frames)


def frame_ingest_multi(frames, y, geoms, filter, a, b, fill=(0.0, 0.0, 0.0), swap_rb=False, y_amax=None):
    """``frame_ingest`` for frames of different sizes, and with an antialiased downscale
    (prpe_frame_ingest_multi, include/prpe.h). ``frames``: a sequence of B uint8 device tensors
    [Hs_i, Ws_i, 3], any strides (a 4-D tensor is taken as its frames). ``geoms``: B regions (top,
    left, nh, nw), a sequence or an int tensor [B, 4] (``FrameIngest.geometry_batch``). ``filter``:
    0 bilinear (``frame_ingest``'s bytes, frame by frame), 1 antialias (torch's triangle filter on
    every axis that shrinks, by at most 32). The table of frames is built here, on the host, and
    travels in the kernel arguments. Every check made here raises ``ValueError``."""
    what = "prpe_frame_ingest_multi"
    frames = frame_list(frames)
    B = len(frames)
    if B < 1:
        raise ValueError(f"{what}: no frames")
    for n, f in enumerate(frames):
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8:
            raise ValueError(f"{what}: frame {n} must be a uint8 tensor, got "
                             f"{getattr(f, 'dtype', type(f).__name__)}")
        if f.dim() != 3 or f.shape[2] != 3 or f.numel() == 0:
            raise ValueError(f"{what}: frame {n} must be [Hs, Ws, 3] (3 channels last), got {list(f.shape)}")
    if filter not in (0, 1):
        raise ValueError(f"{what}: filter must be 0 (bilinear) or 1 (antialias), got {filter!r}")
    geoms = geoms.tolist() if isinstance(geoms, torch.Tensor) else [tuple(g) for g in geoms]
    if len(geoms) != B or any(len(g) != 4 for g in geoms):
        raise ValueError(f"{what}: {B} frames need {B} regions (top, left, nh, nw), got {len(geoms)}")
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 4):
        raise ValueError(f"{what}: y must be a float32 device tensor [B, H, W, 4]")
    if y.shape[0] != B or y.shape[3] != 4 or y.stride(3) != 1 or y.data_ptr() % 16 or \
            any(s % 4 for s in y.stride()[:3]):
        raise ValueError(f"{what}: y must be [{B}, H, W, 4] with 4 contiguous, 16-byte aligned channels, got "
                         f"{list(y.shape)} strides {list(y.stride())}")
    table = (IngestSrc * B)()
    for n, (f, g) in enumerate(zip(frames, geoms)):
        if not f.is_cuda or f.device != y.device:
            raise ValueError(f"{what}: frame {n} must be on {y.device}, got one on {f.device}")
        top, left, nh, nw = (int(v) for v in g)
        if nh < 1 or nw < 1 or top < 0 or left < 0 or top + nh > y.shape[1] or left + nw > y.shape[2]:
            raise ValueError(f"{what}: region {(top, left, nh, nw)} of frame {n} is empty or not inside "
                             f"{list(y.shape[1:3])}")
        Hs, Ws = f.shape[:2]
        if filter and (Hs > INGEST_MAX_SCALE * nh or Ws > INGEST_MAX_SCALE * nw):
            raise ValueError(f"{what}: frame {n}, {Hs} x {Ws} into {nh} x {nw}: the antialias filter shrinks an "
                             f"axis by at most {INGEST_MAX_SCALE}")
        table[n] = IngestSrc(f.data_ptr(), Hs, Ws, *f.stride(), top, left, nh, nw)
    _check_slots(what, B, y_amax)
    check(lib().prpe_frame_ingest_multi(table, B, C.byref(view(y)), int(filter), _f3(what, "a", a),
                                        _f3(what, "b", b), _f3(what, "fill", fill), int(bool(swap_rb)),
                                        _ptr(y_amax), _stream()), what)
    return y


def crop_resize_u8(frames, crop_meta, n_crops, crops, a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0), swap_rb=False):
    """``crop_resize`` from uint8 source frames [B, Hs, Ws, 3] (any strides), every pixel of a
    filled slot then raw * a[c] + b[c] (prpe_crop_resize_u8, include/prpe.h); the windows of
    ``crop_meta`` are in the pixels of these frames."""
    what = "prpe_crop_resize_u8"
    fv = _u8_frames(what, frames)
    if not (isinstance(crop_meta, torch.Tensor) and crop_meta.dim() == 2):
        raise ValueError(f"{what}: crop_meta must be [max_crops, {CROP_META_COLS}]")
    max_crops = crop_meta.shape[0]
    shape = (max_crops, VIT_IMG[0] + 2 * CROP_BORDER, VIT_IMG[1] + 2 * CROP_BORDER, 4)
    _check_dev(what, "crop_meta", crop_meta, torch.float32, (max_crops, CROP_META_COLS))
    _check_dev(what, "n_crops", n_crops, torch.int32, (1,))
    _check_dev(what, "crops", crops, torch.float32, shape)
    if max_crops < 1 or crops.data_ptr() % 16:
        raise ValueError(f"{what}: crops must hold at least one slot and be 16-byte aligned")
    check(lib().prpe_crop_resize_u8(C.byref(fv), crop_meta.data_ptr(), n_crops.data_ptr(), max_crops,
                                    _f3(what, "a", a), _f3(what, "b", b), int(bool(swap_rb)), crops.data_ptr(),
                                    _stream()), what)
    return crops


# ------------------------------------------------------------------ per-face crops and the match (csrc/roi.hip)
ROI_MAX_OUT = 4096                   # largest output side of roi_select / roi_resize
MATCH_MAX_PER_FRAME = 32             # persons / faces per frame face_person_match takes


def roi_select(dets, counts, frame_hw, out_hw, *, crop_meta, n_crops, status, score_thr=0.25, max_per_frame=8,
               min_size=4.0, box_scale=(1.0, 1.0), pad=1.25):
    """``crop_select`` for an ``out_hw`` = (out_h, out_w) output: the window takes the aspect
    out_w / out_h (prpe_roi_select, include/prpe.h). Everything else is ``crop_select``'s; at
    (256, 192) so are the bits. No host read."""
    what = "prpe_roi_select"
    if not (isinstance(dets, torch.Tensor) and dets.dim() == 3 and dets.shape[2] == 6):
        raise ValueError(f"{what}: dets must be [B, max_det, 6]")
    B, max_det, _ = dets.shape
    _check_dev(what, "dets", dets, torch.float32, (B, max_det, 6))
    _check_dev(what, "counts", counts, torch.int32, (B,))
    if not (isinstance(crop_meta, torch.Tensor) and crop_meta.dim() == 2):
        raise ValueError(f"{what}: crop_meta must be [max_crops, {CROP_META_COLS}]")
    max_crops = crop_meta.shape[0]
    _check_dev(what, "crop_meta", crop_meta, torch.float32, (max_crops, CROP_META_COLS))
    _check_dev(what, "n_crops", n_crops, torch.int32, (1,))
    _check_dev(what, "status", status, torch.int32, (1,))
    H, W = (int(v) for v in frame_hw)
    oh, ow = (int(v) for v in out_hw)
    sx, sy = (float(v) for v in box_scale)
    if B < 1 or max_det < 1 or max_crops < 1 or max_per_frame < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: empty batch, crop list or frame")
    if not (1 <= oh <= ROI_MAX_OUT and 1 <= ow <= ROI_MAX_OUT):
        raise ValueError(f"{what}: the output size {(oh, ow)} must be within 1..{ROI_MAX_OUT}")
    check(lib().prpe_roi_select(dets.data_ptr(), counts.data_ptr(), B, max_det, float(score_thr), int(max_per_frame),
                                float(min_size), sx, sy, H, W, float(pad), oh, ow, max_crops, crop_meta.data_ptr(),
                                n_crops.data_ptr(), status.data_ptr(), _stream()), what)
    return crop_meta, n_crops, status


def _roi_args(what, crop_meta, n_crops, y, y_amax):
    """The checks roi_resize and roi_resize_u8 share; returns max_crops."""
    if not (isinstance(crop_meta, torch.Tensor) and crop_meta.dim() == 2):
        raise ValueError(f"{what}: crop_meta must be [max_crops, {CROP_META_COLS}]")
    max_crops = crop_meta.shape[0]
    _check_dev(what, "crop_meta", crop_meta, torch.float32, (max_crops, CROP_META_COLS))
    _check_dev(what, "n_crops", n_crops, torch.int32, (1,))
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 4):
        raise ValueError(f"{what}: y must be a float32 device tensor [max_crops, out_h, out_w, 4]")
    if max_crops < 1 or y.shape[0] != max_crops or y.shape[3] != 4 or y.stride(3) != 1 or y.data_ptr() % 16 or \
            any(s % 4 for s in y.stride()[:3]) or not (1 <= y.shape[1] <= ROI_MAX_OUT and 1 <= y.shape[2] <= ROI_MAX_OUT):
        raise ValueError(f"{what}: y must be [{max_crops}, out_h, out_w, 4] (sides 1..{ROI_MAX_OUT}) with 4 contiguous, "
                         f"16-byte aligned channels, got {list(y.shape)} strides {list(y.stride())}")
    _check_slots(what, max_crops, y_amax)
    return max_crops


def roi_resize(frames, crop_meta, n_crops, y, y_amax=None):
    """Resample the windows of ``crop_meta`` from ``frames`` ([B, 3, H, W] float32 device, any
    strides) into ``y`` [max_crops, out_h, out_w, 4], the interior of a zero-bordered NHWC4 buffer
    (Engine.face_stem_buf's, Engine.crop_pix4's; prpe_roi_resize, include/prpe.h). Slots at or
    past n_crops are zeroed. ``y_amax`` ([max_crops] device, zeroed): raised to max|y[s]| per slot."""
    what = "prpe_roi_resize"
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.float32 and
            frames.dim() == 4 and frames.shape[1] == 3 and frames.numel() > 0):
        raise ValueError(f"{what}: frames must be a float32 device tensor [B, 3, H, W]")
    max_crops = _roi_args(what, crop_meta, n_crops, y, y_amax)
    check(lib().prpe_roi_resize(C.byref(view(nhwc(frames))), crop_meta.data_ptr(), n_crops.data_ptr(), max_crops,
                                C.byref(view(y)), _ptr(y_amax), _stream()), what)
    return y


def roi_resize_u8(frames, crop_meta, n_crops, y, a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0), swap_rb=False, y_amax=None):
    """``roi_resize`` from uint8 source frames [B, Hs, Ws, 3] (any strides), every pixel of a
    filled slot then raw * a[c] + b[c] (prpe_roi_resize_u8, include/prpe.h); the windows of
    ``crop_meta`` are in the pixels of these frames."""
    what = "prpe_roi_resize_u8"
    fv = _u8_frames(what, frames)
    max_crops = _roi_args(what, crop_meta, n_crops, y, y_amax)
    check(lib().prpe_roi_resize_u8(C.byref(fv), crop_meta.data_ptr(), n_crops.data_ptr(), max_crops,
                                   _f3(what, "a", a), _f3(what, "b", b), int(bool(swap_rb)), C.byref(view(y)),
                                   _ptr(y_amax), _stream()), what)
    return y


def face_person_match(crop_meta_p, n_p, keypoints, crop_meta_f, n_f, ident, score, n_frames, *, face_slot,
                      person_ident, person_score, status, kp_thr=0.3, head_kpts=5):
    """Identities to skeletons (prpe_face_person_match, include/prpe.h): the person list
    (crop_meta_p [P, 8], n_p [1], keypoints [P, K, 3] in frame pixels) and the face list
    (crop_meta_f [F, 8], n_f [1], ident [F] int64, score [F]) of the same ``n_frames`` frames ->
    per person slot face_slot [P] int32, person_ident [P] int64, person_score [P]; status
    [n_frames] int32 (1: more than 32 persons or faces in the frame, no matches there). A face goes
    to the person whose head point (mean of the first ``head_kpts`` keypoints with score >=
    ``kp_thr``) is nearest among the persons whose window holds the face centre, greedily and
    one-to-one. No host read."""
    what = "prpe_face_person_match"
    for name, t in (("crop_meta_p", crop_meta_p), ("crop_meta_f", crop_meta_f)):
        if not (isinstance(t, torch.Tensor) and t.dim() == 2):
            raise ValueError(f"{what}: {name} must be [slots, {CROP_META_COLS}]")
    if not (isinstance(keypoints, torch.Tensor) and keypoints.dim() == 3 and keypoints.shape[2] == 3):
        raise ValueError(f"{what}: keypoints must be [P, K, 3]")
    P, F = crop_meta_p.shape[0], crop_meta_f.shape[0]
    K, B = keypoints.shape[1], int(n_frames)
    _check_dev(what, "crop_meta_p", crop_meta_p, torch.float32, (P, CROP_META_COLS))
    _check_dev(what, "n_p", n_p, torch.int32, (1,))
    _check_dev(what, "keypoints", keypoints, torch.float32, (P, K, 3))
    _check_dev(what, "crop_meta_f", crop_meta_f, torch.float32, (F, CROP_META_COLS))
    _check_dev(what, "n_f", n_f, torch.int32, (1,))
    _check_dev(what, "ident", ident, torch.int64, (F,))
    _check_dev(what, "score", score, torch.float32, (F,))
    _check_dev(what, "face_slot", face_slot, torch.int32, (P,))
    _check_dev(what, "person_ident", person_ident, torch.int64, (P,))
    _check_dev(what, "person_score", person_score, torch.float32, (P,))
    _check_dev(what, "status", status, torch.int32, (max(B, 0),))
    head_kpts, kp_thr = int(head_kpts), float(kp_thr)
    if P < 1 or F < 1 or B < 1 or K < 1 or not 1 <= head_kpts <= K or kp_thr != kp_thr:
        raise ValueError(f"{what}: P = {P}, F = {F}, frames = {B}, head_kpts = {head_kpts} of K = {K}, "
                         f"kp_thr = {kp_thr}")
    check(lib().prpe_face_person_match(crop_meta_p.data_ptr(), n_p.data_ptr(), P, keypoints.data_ptr(), K,
                                       crop_meta_f.data_ptr(), n_f.data_ptr(), F, ident.data_ptr(), score.data_ptr(),
                                       kp_thr, head_kpts, B, face_slot.data_ptr(), person_ident.data_ptr(),
                                       person_score.data_ptr(), status.data_ptr(), _stream()), what)
    return face_slot, person_ident, person_score, status


# ------------------------------------------------------------------ aligned face crops (csrc/facealign.hip)
WARP_COLS = 8                        # flag, person slot, a, b, tx, c, d, ty


def face_align_fit(crop_meta_f, n_f, n_p, keypoints, person_face, out_hw, *, warp, kp_thr=0.3, scale=(0.5, 2.0)):
    """The similarity that puts each matched person's eyes and nose (keypoints [P, K, 3] in frame
    pixels; COCO 2, 1, 0) on the ArcFace template of an ``out_hw`` crop -> ``warp`` [F, 8], the
    face list's rows for prpe_roi_warp (prpe_face_align_fit, include/prpe.h). ``person_face`` [P]
    int32 is ``face_person_match``'s face_slot; ``warp`` must be zeroed by the caller: only the
    rows that pass the gates (``kp_thr``, ``scale`` = (lo, hi) of crop width over window width, the
    crop centre inside the window) are written. No host read."""
    what = "prpe_face_align_fit"
    if not (isinstance(crop_meta_f, torch.Tensor) and crop_meta_f.dim() == 2):
        raise ValueError(f"{what}: crop_meta_f must be [F, {CROP_META_COLS}]")
    if not (isinstance(keypoints, torch.Tensor) and keypoints.dim() == 3 and keypoints.shape[2] == 3):
        raise ValueError(f"{what}: keypoints must be [P, K, 3]")
    F, (P, K, _) = crop_meta_f.shape[0], keypoints.shape
    _check_dev(what, "crop_meta_f", crop_meta_f, torch.float32, (F, CROP_META_COLS))
    _check_dev(what, "n_f", n_f, torch.int32, (1,))
    _check_dev(what, "n_p", n_p, torch.int32, (1,))
    _check_dev(what, "keypoints", keypoints, torch.float32, (P, K, 3))
    _check_dev(what, "person_face", person_face, torch.int32, (P,))
    _check_dev(what, "warp", warp, torch.float32, (F, WARP_COLS))
    oh, ow = (int(v) for v in out_hw)
    lo, hi = (float(v) for v in scale)
    kp_thr = float(kp_thr)
    if P < 1 or F < 1 or K < 3 or kp_thr != kp_thr or not 0.0 < lo <= hi:
        raise ValueError(f"{what}: P = {P}, F = {F}, K = {K} (at least 3), kp_thr = {kp_thr}, scale = {(lo, hi)} "
                         f"(0 < lo <= hi)")
    if not (1 <= oh <= ROI_MAX_OUT and 1 <= ow <= ROI_MAX_OUT):
        raise ValueError(f"{what}: the output size {(oh, ow)} must be within 1..{ROI_MAX_OUT}")
    check(lib().prpe_face_align_fit(crop_meta_f.data_ptr(), n_f.data_ptr(), F, n_p.data_ptr(), P, keypoints.data_ptr(),
                                    K, person_face.data_ptr(), oh, ow, kp_thr, lo, hi, warp.data_ptr(), _stream()),
          what)
    return warp


def roi_warp(frames, crop_meta, n_crops, warp, y, y_amax=None):
    """``roi_resize`` with ``warp`` [max_crops, 8] (``face_align_fit``'s): a slot whose row is
    flagged is sampled along the row's affine map, every other slot from its window with
    ``roi_resize``'s bits (prpe_roi_warp, include/prpe.h)."""
    what = "prpe_roi_warp"
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.float32 and
            frames.dim() == 4 and frames.shape[1] == 3 and frames.numel() > 0):
        raise ValueError(f"{what}: frames must be a float32 device tensor [B, 3, H, W]")
    max_crops = _roi_args(what, crop_meta, n_crops, y, y_amax)
    _check_dev(what, "warp", warp, torch.float32, (max_crops, WARP_COLS))
    check(lib().prpe_roi_warp(C.byref(view(nhwc(frames))), crop_meta.data_ptr(), n_crops.data_ptr(), max_crops,
                              warp.data_ptr(), C.byref(view(y)), _ptr(y_amax), _stream()), what)
    return y


def roi_warp_u8(frames, crop_meta, n_crops, warp, y, a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0), swap_rb=False,
                y_amax=None):
    """``roi_warp`` from uint8 source frames [B, Hs, Ws, 3] (any strides) with ``roi_resize_u8``'s
    a, b and channel order (prpe_roi_warp_u8, include/prpe.h)."""
    what = "prpe_roi_warp_u8"
    fv = _u8_frames(what, frames)
    max_crops = _roi_args(what, crop_meta, n_crops, y, y_amax)
    _check_dev(what, "warp", warp, torch.float32, (max_crops, WARP_COLS))
    check(lib().prpe_roi_warp_u8(C.byref(fv), crop_meta.data_ptr(), n_crops.data_ptr(), max_crops, warp.data_ptr(),
                                 _f3(what, "a", a), _f3(what, "b", b), int(bool(swap_rb)), C.byref(view(y)),
                                 _ptr(y_amax), _stream()), what)
    return y


# ------------------------------------------------------------------ NV12 frames in (csrc/nv12.hip)
def _nv12_frames(what, frames):
    """(prpe_nv12, coef) of a prpe.NV12Frames: the class has checked shapes, dtypes and strides;
    the device is checked here, before the C ABI."""
    from .nv12 import NV12Frames
    if not isinstance(frames, NV12Frames):
        raise ValueError(f"{what}: frames must be a prpe.NV12Frames, got {type(frames).__name__}")
    if not frames.is_cuda:
        raise ValueError(f"{what}: the planes must be HIP device tensors, got them on {frames.device}")
    B, Hs, Ws = frames.shape
    src = NV12(frames.y.data_ptr(), frames.uv.data_ptr(), B, Hs, Ws, frames.y.stride(0), frames.y.stride(1),
               frames.uv.stride(0), frames.uv.stride(1))
    return src, (C.c_int32 * 6)(*(int(v) for v in frames.coef))


def nv12_to_rgb(frames, out, swap_rb=False):
    """NV12 frames -> ``out``, uint8 [B, Hs, Ws, 3] on the device with 3 contiguous bytes per pixel
    and any row and frame strides; ``swap_rb`` writes B, G, R (prpe_nv12_to_rgb, include/prpe.h)."""
    what = "prpe_nv12_to_rgb"
    src, coef = _nv12_frames(what, frames)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda:
        raise ValueError(f"{what}: out must be a uint8 device tensor")
    if tuple(out.shape) != frames.shape + (3,) or out.stride(3) != 1 or out.stride(2) != 3 or \
            out.stride(1) < 3 * frames.shape[2]:
        raise ValueError(f"{what}: out must be {list(frames.shape + (3,))} with packed pixels (strides (.., .., 3, 1)), "
                         f"got {list(out.shape)} strides {list(out.stride())}")
    check(lib().prpe_nv12_to_rgb(C.byref(src), coef, int(bool(swap_rb)), out.data_ptr(), out.stride(0), out.stride(1),
                                 _stream()), what)
    return out


def frame_ingest_nv12(frames, y, region, a, b, fill=(0.0, 0.0, 0.0), y_amax=None):
    """``frame_ingest`` from NV12 frames (a prpe.NV12Frames): every tap converted as it is gathered;
    the output channels are R, G, B (prpe_frame_ingest_nv12, include/prpe.h)."""
    what = "prpe_frame_ingest_nv12"
    src, coef = _nv12_frames(what, frames)
    B = frames.shape[0]
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 4):
        raise ValueError(f"{what}: y must be a float32 device tensor [B, H, W, 4]")
    if y.shape[0] != B or y.shape[3] != 4 or y.stride(3) != 1 or y.data_ptr() % 16 or \
            any(s % 4 for s in y.stride()[:3]):
        raise ValueError(f"{what}: y must be [{B}, H, W, 4] with 4 contiguous, 16-byte aligned "
                         f"channels, got {list(y.shape)} strides {list(y.stride())}")
    top, left, nh, nw = (int(v) for v in region)
    if nh < 1 or nw < 1 or top < 0 or left < 0 or top + nh > y.shape[1] or left + nw > y.shape[2]:
        raise ValueError(f"{what}: region {(top, left, nh, nw)} is empty or not inside {list(y.shape[1:3])}")
    _check_slots(what, B, y_amax)
    check(lib().prpe_frame_ingest_nv12(C.byref(src), coef, C.byref(view(y)), top, left, nh, nw, _f3(what, "a", a),
                                       _f3(what, "b", b), _f3(what, "fill", fill), _ptr(y_amax), _stream()), what)
    return y


def crop_resize_nv12(frames, crop_meta, n_crops, crops, a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0)):
    """``crop_resize_u8`` from NV12 frames (prpe_crop_resize_nv12, include/prpe.h)."""
    what = "prpe_crop_resize_nv12"
    src, coef = _nv12_frames(what, frames)
    if not (isinstance(crop_meta, torch.Tensor) and crop_meta.dim() == 2):
        raise ValueError(f"{what}: crop_meta must be [max_crops, {CROP_META_COLS}]")
    max_crops = crop_meta.shape[0]
    shape = (max_crops, VIT_IMG[0] + 2 * CROP_BORDER, VIT_IMG[1] + 2 * CROP_BORDER, 4)
    _check_dev(what, "crop_meta", crop_meta, torch.float32, (max_crops, CROP_META_COLS))
    _check_dev(what, "n_crops", n_crops, torch.int32, (1,))
    _check_dev(what, "crops", crops, torch.float32, shape)
    if max_crops < 1 or crops.data_ptr() % 16:
        raise ValueError(f"{what}: crops must hold at least one slot and be 16-byte aligned")
    check(lib().prpe_crop_resize_nv12(C.byref(src), coef, crop_meta.data_ptr(), n_crops.data_ptr(), max_crops,
                                      _f3(what, "a", a), _f3(what, "b", b), crops.data_ptr(), _stream()), what)
    return crops


def roi_resize_nv12(frames, crop_meta, n_crops, y, a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0), y_amax=None):
    """``roi_resize_u8`` from NV12 frames (prpe_roi_resize_nv12, include/prpe.h)."""
    what = "prpe_roi_resize_nv12"
    src, coef = _nv12_frames(what, frames)
    max_crops = _roi_args(what, crop_meta, n_crops, y, y_amax)
    check(lib().prpe_roi_resize_nv12(C.byref(src), coef, crop_meta.data_ptr(), n_crops.data_ptr(), max_crops,
                                     C.byref(view(y)), _f3(what, "a", a), _f3(what, "b", b), _ptr(y_amax),
                                     _stream()), what)
    return y


def roi_warp_nv12(frames, crop_meta, n_crops, warp, y, a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0), y_amax=None):
    """``roi_warp_u8`` from NV12 frames (prpe_roi_warp_nv12, include/prpe.h)."""
    what = "prpe_roi_warp_nv12"
    src, coef = _nv12_frames(what, frames)
    max_crops = _roi_args(what, crop_meta, n_crops, y, y_amax)
    _check_dev(what, "warp", warp, torch.float32, (max_crops, WARP_COLS))
    check(lib().prpe_roi_warp_nv12(C.byref(src), coef, crop_meta.data_ptr(), n_crops.data_ptr(), max_crops,
                                   warp.data_ptr(), C.byref(view(y)), _f3(what, "a", a), _f3(what, "b", b),
                                   _ptr(y_amax), _stream()), what)
    return y


# ------------------------------------------------------------------ annotated frames out (csrc/annotate.hip)
ANNOTATE_MAX_SIDE = 16384
ANNOTATE_MAX_K = 64
ANNOTATE_MAX_LIMBS = 32
ANNOTATE_MAX_R = 16                  # box_t, limb_r, kp_r
ANNOTATE_BLOCKS = 17                 # pixelation blocks per side of a face, at most
ANNOTATE_MAX_SLOTS = 1 << 20
# the COCO skeleton: 19 limbs over the 17 keypoints
COCO_LIMBS = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9),
              (8, 10), (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))


def annotate_geometry():
    """(tile h, tile w, super-tile h, super-tile w) of the paint launch (prpe_annotate_geometry)."""
    out = (C.c_int32 * 4)()
    lib().prpe_annotate_geometry(out)
    return tuple(out)


def annotate_table_bytes(max_p, max_f, K, n_limbs):
    """Bytes of the primitive table of an annotate call (prpe_annotate_table_bytes)."""
    n = lib().prpe_annotate_table_bytes(int(max_p), int(max_f), int(K), int(n_limbs))
    if n < 0:
        raise ValueError(f"prpe_annotate_table_bytes: max_p = {max_p}, max_f = {max_f} (0..{ANNOTATE_MAX_SLOTS}), "
                         f"K = {K} (1..{ANNOTATE_MAX_K}), limbs = {n_limbs} (0..{ANNOTATE_MAX_LIMBS})")
    return n


def annotate_workspaces(max_p, max_f, K, n_limbs, device):
    """(table, means) for an annotate call of these sizes: uint8 device tensors the caller keeps."""
    table = torch.empty(max(annotate_table_bytes(max_p, max_f, K, n_limbs), 16), dtype=torch.uint8, device=device)
    means = torch.empty(max(max_f, 1), ANNOTATE_BLOCKS, ANNOTATE_BLOCKS, 4, dtype=torch.uint8, device=device)
    return table, means


def _annotate_args(what, dev, hw, crop_meta_p, n_p, keypoints, person_colour, crop_meta_f, n_f, face_mode, face_colour,
                   palette, limbs, table, means, box_t, limb_r, kp_r, kp_thr, cell, scale):
    """prpe_annotate_args after every check the C side makes (and the shapes it cannot see)."""
    def on_dev(name, t, dtype, shape):
        _check_dev(what, name, t, dtype, shape)
        if t.device != dev:
            raise ValueError(f"{what}: {name} is on {t.device}, the surface on {dev}")

    H, W = hw
    if not (1 <= H <= ANNOTATE_MAX_SIDE and 1 <= W <= ANNOTATE_MAX_SIDE):
        raise ValueError(f"{what}: the surface's sides must be in 1..{ANNOTATE_MAX_SIDE}, got {H} x {W}")
    max_p = max_f = 0
    K = 1
    if crop_meta_p is not None:
        if not (isinstance(crop_meta_p, torch.Tensor) and crop_meta_p.dim() == 2):
            raise ValueError(f"{what}: crop_meta_p must be [max_p, {CROP_META_COLS}]")
        if not (isinstance(keypoints, torch.Tensor) and keypoints.dim() == 3 and keypoints.shape[2] == 3):
            raise ValueError(f"{what}: keypoints must be [max_p, K, 3]")
        max_p, K = crop_meta_p.shape[0], keypoints.shape[1]
        if not (1 <= max_p <= ANNOTATE_MAX_SLOTS and 1 <= K <= ANNOTATE_MAX_K):
            raise ValueError(f"{what}: max_p = {max_p} (1..{ANNOTATE_MAX_SLOTS}), K = {K} (1..{ANNOTATE_MAX_K})")
        on_dev("crop_meta_p", crop_meta_p, torch.float32, (max_p, CROP_META_COLS))
        on_dev("n_p", n_p, torch.int32, (1,))
        on_dev("keypoints", keypoints, torch.float32, (max_p, K, 3))
        on_dev("person_colour", person_colour, torch.int32, (max_p,))
    if crop_meta_f is not None:
        if not (isinstance(crop_meta_f, torch.Tensor) and crop_meta_f.dim() == 2):
            raise ValueError(f"{what}: crop_meta_f must be [max_f, {CROP_META_COLS}]")
        max_f = crop_meta_f.shape[0]
        if not 1 <= max_f <= ANNOTATE_MAX_SLOTS:
            raise ValueError(f"{what}: max_f = {max_f} (1..{ANNOTATE_MAX_SLOTS})")
        on_dev("crop_meta_f", crop_meta_f, torch.float32, (max_f, CROP_META_COLS))
        on_dev("n_f", n_f, torch.int32, (1,))
        on_dev("face_mode", face_mode, torch.int32, (max_f,))
        on_dev("face_colour", face_colour, torch.int32, (max_f,))
    if not (isinstance(palette, torch.Tensor) and palette.dim() == 2 and palette.shape[0] >= 1):
        raise ValueError(f"{what}: palette must be [n_colours, 4] with at least one colour")
    n_colours = palette.shape[0]
    on_dev("palette", palette, torch.uint8, (n_colours, 4))
    if palette.data_ptr() % 4:
        raise ValueError(f"{what}: palette must be 4-byte aligned")
    limbs = [(int(a), int(b)) for a, b in limbs] if max_p else []       # no persons: no skeleton to index
    if len(limbs) > ANNOTATE_MAX_LIMBS or any(not (0 <= v < K) for ab in limbs for v in ab):
        raise ValueError(f"{what}: at most {ANNOTATE_MAX_LIMBS} limbs with keypoint indices in [0, {K})")
    box_t, limb_r, kp_r, cell, kp_thr = int(box_t), int(limb_r), int(kp_r), int(cell), float(kp_thr)
    if not all(0 <= v <= ANNOTATE_MAX_R for v in (box_t, limb_r, kp_r)):
        raise ValueError(f"{what}: box_t = {box_t}, limb_r = {limb_r}, kp_r = {kp_r} must be in 0..{ANNOTATE_MAX_R}")
    if not 2 <= cell <= 64 or cell % 2:
        raise ValueError(f"{what}: cell must be even and in 2..64, got {cell}")
    sx, sy = (float(v) for v in ((scale, scale) if isinstance(scale, (int, float)) else scale))
    if not (0.0 < sx < float("inf") and 0.0 < sy < float("inf")) or kp_thr != kp_thr:
        raise ValueError(f"{what}: sx = {sx}, sy = {sy} must be finite and positive and kp_thr = {kp_thr} a number")
    need = annotate_table_bytes(max_p, max_f, K, len(limbs))
    tb = 0
    if max_p + max_f:
        if not (isinstance(table, torch.Tensor) and table.dtype == torch.uint8 and table.is_contiguous() and
                table.device == dev and table.numel() >= need and table.data_ptr() % 16 == 0):
            raise ValueError(f"{what}: table must be a contiguous uint8 tensor of at least {need} bytes on {dev}, "
                             "16-byte aligned (ops.annotate_workspaces)")
        tb = table.numel()
    if max_f:
        on_dev("means", means, torch.uint8, (max_f, ANNOTATE_BLOCKS, ANNOTATE_BLOCKS, 4))
        if means.data_ptr() % 4:
            raise ValueError(f"{what}: means must be 4-byte aligned")
    flat = (C.c_int32 * max(2 * len(limbs), 1))(*(v for ab in limbs for v in ab))
    args = AnnotateArgs(_ptr(crop_meta_p), _ptr(n_p), _ptr(keypoints), _ptr(person_colour), _ptr(crop_meta_f), _ptr(n_f),
                        _ptr(face_mode), _ptr(face_colour), palette.data_ptr(), flat,
                        table.data_ptr() if tb else None, means.data_ptr() if max_f else None, tb,
                        max_p, K, max_f, n_colours, len(limbs), box_t, limb_r, kp_r, cell, kp_thr, sx, sy)
    return args, flat


def _annotate(what, call, dst, dev, hw, persons, faces, palette, limbs, table, means, kw):
    crop_meta_p, n_p, keypoints, person_colour = persons if persons is not None else (None,) * 4
    crop_meta_f, n_f, face_mode, face_colour = faces if faces is not None else (None,) * 4
    args, keep = _annotate_args(what, dev, hw, crop_meta_p, n_p, keypoints, person_colour, crop_meta_f, n_f, face_mode,
                                face_colour, palette, limbs, table, means, **kw)
    check(call(C.byref(dst), C.byref(args), _stream()), what)
    del keep


def annotate_nv12(frames, palette, *, persons=None, faces=None, limbs=COCO_LIMBS, table=None, means=None, box_t=2,
                  limb_r=1, kp_r=2, kp_thr=0.3, cell=8, scale=1.0):
    """Paint skeletons, boxes and face redaction IN PLACE into NV12 frames (a prpe.NV12Frames;
    prpe_annotate_nv12, include/prpe.h). ``persons`` = (crop_meta [max_p, 8], n_p [1] int32,
    keypoints [max_p, K, 3], person_colour [max_p] int32; negative: not drawn) and ``faces`` =
    (crop_meta [max_f, 8], n_f [1] int32, face_mode [max_f] int32: 1 pixelate, 2 fill,
    face_colour [max_f] int32), either may be None. ``palette``: uint8 [n, 4] device = (Y, U, V, 0).
    ``limbs``: pairs of keypoint indices (host). ``table``, ``means``: ops.annotate_workspaces.
    ``scale``: (sx, sy), list coordinates -> surface pixels. No state, no host read."""
    what = "prpe_annotate_nv12"
    src, _ = _nv12_frames(what, frames)
    _annotate(what, lib().prpe_annotate_nv12, src, frames.device, frames.shape[1:], persons, faces, palette, limbs, table,
              means, dict(box_t=box_t, limb_r=limb_r, kp_r=kp_r, kp_thr=kp_thr, cell=cell, scale=scale))
    return frames


def annotate_u8(frames, palette, *, persons=None, faces=None, limbs=COCO_LIMBS, table=None, means=None, box_t=2,
                limb_r=1, kp_r=2, kp_thr=0.3, cell=8, scale=1.0):
    """``annotate_nv12`` on uint8 frames [B, H, W, 3] with any strides; ``palette`` holds
    (c0, c1, c2, 0) in the frames' channel order (prpe_annotate_u8, include/prpe.h)."""
    what = "prpe_annotate_u8"
    fv = _u8_frames(what, frames)
    _annotate(what, lib().prpe_annotate_u8, fv, frames.device, frames.shape[1:3], persons, faces, palette, limbs, table,
              means, dict(box_t=box_t, limb_r=limb_r, kp_r=kp_r, kp_thr=kp_thr, cell=cell, scale=scale))
    return frames


# ------------------------------------------------------------------ tracking across frames (csrc/track.hip)
TRACK_SLOTS = 32                     # track slots per stream, and persons per frame track_update takes
TRACK_MAX_K = 64                     # keypoints per person
TRACK_MODES = {"iou": 0, "pose": 1}


def track_update(crop_meta_p, n_p, keypoints, person_ident, person_score, frame_stream, *, trk_meta, trk_kpts,
                 trk_ident, trk_iscore, next_id, track_id, track_hits, track_ident, track_iscore, status, k2,
                 mode="iou", gate=0.7, kp_thr=0.3, min_common=3, new_thr=0.25, max_age=30):
    """Persons to tracks (prpe_track_update, include/prpe.h): the person list (crop_meta_p [P, 8],
    n_p [1], keypoints [P, K, 3] in frame pixels, person_ident [P] int64, person_score [P]) of B
    frames whose streams are ``frame_stream`` [B] int32 (outside [0, S): not tracked), against the
    caller's state of S streams x 32 slots (trk_meta [S, 32, 8], trk_kpts [S, 32, K, 3], trk_ident
    [S, 32] int64, trk_iscore [S, 32], next_id [S] int32), updated in place -> per person slot
    track_id, track_hits [P] int32, track_ident [P] int64, track_iscore [P]; status [B] int32
    (1: more than 32 persons, the frame is skipped; 2: no free slot for a new track). ``mode``:
    "iou" (cost 1 - IoU of the windows) or "pose" (mean squared keypoint distance over area *
    k2[k]); ``k2``: K host floats, (2 sigma_k)^2. One wavefront per stream walks its frames in
    ascending order; no host read."""
    what = "prpe_track_update"
    if not (isinstance(crop_meta_p, torch.Tensor) and crop_meta_p.dim() == 2):
        raise ValueError(f"{what}: crop_meta_p must be [slots, {CROP_META_COLS}]")
    if not (isinstance(keypoints, torch.Tensor) and keypoints.dim() == 3 and keypoints.shape[2] == 3):
        raise ValueError(f"{what}: keypoints must be [P, K, 3]")
    if not (isinstance(frame_stream, torch.Tensor) and frame_stream.dim() == 1):
        raise ValueError(f"{what}: frame_stream must be [B]")
    if not (isinstance(trk_meta, torch.Tensor) and trk_meta.dim() == 3):
        raise ValueError(f"{what}: trk_meta must be [S, {TRACK_SLOTS}, 8]")
    if mode not in TRACK_MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(TRACK_MODES)}, got {mode!r}")
    P, K, B, S = crop_meta_p.shape[0], keypoints.shape[1], frame_stream.shape[0], trk_meta.shape[0]
    T = TRACK_SLOTS
    _check_dev(what, "crop_meta_p", crop_meta_p, torch.float32, (P, CROP_META_COLS))
    _check_dev(what, "n_p", n_p, torch.int32, (1,))
    _check_dev(what, "keypoints", keypoints, torch.float32, (P, K, 3))
    _check_dev(what, "person_ident", person_ident, torch.int64, (P,))
    _check_dev(what, "person_score", person_score, torch.float32, (P,))
    _check_dev(what, "frame_stream", frame_stream, torch.int32, (B,))
    _check_dev(what, "trk_meta", trk_meta, torch.float32, (S, T, 8))
    _check_dev(what, "trk_kpts", trk_kpts, torch.float32, (S, T, K, 3))
    _check_dev(what, "trk_ident", trk_ident, torch.int64, (S, T))
    _check_dev(what, "trk_iscore", trk_iscore, torch.float32, (S, T))
    _check_dev(what, "next_id", next_id, torch.int32, (S,))
    _check_dev(what, "track_id", track_id, torch.int32, (P,))
    _check_dev(what, "track_hits", track_hits, torch.int32, (P,))
    _check_dev(what, "track_ident", track_ident, torch.int64, (P,))
    _check_dev(what, "track_iscore", track_iscore, torch.float32, (P,))
    _check_dev(what, "status", status, torch.int32, (B,))
    k2 = [float(v) for v in k2]
    gate, kp_thr, new_thr, min_common, max_age = float(gate), float(kp_thr), float(new_thr), int(min_common), int(max_age)
    if P < 1 or B < 1 or S < 1 or not 1 <= K <= TRACK_MAX_K or len(k2) != K:
        raise ValueError(f"{what}: P = {P}, frames = {B}, streams = {S}, K = {K} (1..{TRACK_MAX_K}) with {len(k2)} k2")
    if gate != gate or kp_thr != kp_thr or new_thr != new_thr or not 1 <= min_common <= K or max_age < 0:
        raise ValueError(f"{what}: gate = {gate}, kp_thr = {kp_thr}, new_thr = {new_thr}, min_common = {min_common} "
                         f"of K = {K}, max_age = {max_age}")
    if not all(0.0 < v < float("inf") for v in k2):
        raise ValueError(f"{what}: every k2 must be finite and positive")
    check(lib().prpe_track_update(crop_meta_p.data_ptr(), n_p.data_ptr(), P, keypoints.data_ptr(), K,
                                  person_ident.data_ptr(), person_score.data_ptr(), frame_stream.data_ptr(), B, S,
                                  TRACK_MODES[mode], gate, kp_thr, min_common, (C.c_float * K)(*k2), new_thr, max_age,
                                  trk_meta.data_ptr(), trk_kpts.data_ptr(), trk_ident.data_ptr(),
                                  trk_iscore.data_ptr(), next_id.data_ptr(), track_id.data_ptr(),
                                  track_hits.data_ptr(), track_ident.data_ptr(), track_iscore.data_ptr(),
                                  status.data_ptr(), _stream()), what)
    return track_id, track_hits, track_ident, track_iscore, status


# ------------------------------------------------------------------ track-level face templates (csrc/tracktemplate.hip)
TEMPLATE_WEIGHTS = {"norm": 0, "uniform": 1}
TEMPLATE_SCALE_BITS = 24             # a contribution is llrintf(w * e * 2^24)
TEMPLATE_MAX_NORM = 32768.0          # a face whose norm is at or above 2^15 is skipped
TEMPLATE_MAX_FACES = 1 << 20         # faces a template sums at most
TEMPLATE_MAX_STREAMS = 4096          # the list launch reads S * 32 flags in each of its S workgroups


def _template_persons(what, crop_meta_p, n_p, track_id, frame_stream, trk_meta):
    if not (isinstance(crop_meta_p, torch.Tensor) and crop_meta_p.dim() == 2):
        raise ValueError(f"{what}: crop_meta_p must be [slots, {CROP_META_COLS}]")
    if not (isinstance(frame_stream, torch.Tensor) and frame_stream.dim() == 1):
        raise ValueError(f"{what}: frame_stream must be [B]")
    if not (isinstance(trk_meta, torch.Tensor) and trk_meta.dim() == 3):
        raise ValueError(f"{what}: trk_meta must be [S, {TRACK_SLOTS}, 8]")
    P, B, S = crop_meta_p.shape[0], frame_stream.shape[0], trk_meta.shape[0]
    _check_dev(what, "crop_meta_p", crop_meta_p, torch.float32, (P, CROP_META_COLS))
    _check_dev(what, "n_p", n_p, torch.int32, (1,))
    _check_dev(what, "track_id", track_id, torch.int32, (P,))
    _check_dev(what, "frame_stream", frame_stream, torch.int32, (B,))
    _check_dev(what, "trk_meta", trk_meta, torch.float32, (S, TRACK_SLOTS, 8))
    if P < 1 or B < 1 or not 1 <= S <= TEMPLATE_MAX_STREAMS or P > 1 << 30:
        raise ValueError(f"{what}: P = {P}, frames = {B}, streams = {S}")
    return P, B, S


def track_template_update(crop_meta_p, n_p, track_id, person_face, embeddings, norms, n_f, frame_stream, trk_meta, *,
                          tmpl_owner, tmpl_sum, tmpl_n, tmpl_ident, tmpl_score, dirty_rows, n_dirty, dirty_pos, queries,
                          weight="norm", min_norm=0.0):
    """The faces of this call's persons into their tracks' templates (prpe_track_template_update,
    include/prpe.h), after ``track_update`` of the same call: the person list (crop_meta_p [P, 8],
    n_p [1], track_id [P] int32, person_face [P] int32), the face list (embeddings [F, D] float32 with
    unit stride along D and any row stride >= D, norms [F], n_f [1]), frame_stream [B] int32 and
    trk_meta [S, 32, 8] (read only), against the caller's template state (tmpl_owner, tmpl_n [S, 32]
    int32, tmpl_sum [S, 32, D] int64, tmpl_ident [S, 32] int64, tmpl_score [S, 32]), updated in place
    -> the list of the templates that changed: dirty_rows [Q] int32, n_dirty [1], dirty_pos [S, 32]
    int32 and queries [Q, D] float32 (rows at and past n_dirty zero), Q >= min(S * 32, F).
    ``weight``: "norm" (a face weighs its feature norm) or "uniform"; a face whose norm is below
    ``min_norm`` is skipped. No host read."""
    what = "prpe_track_template_update"
    P, B, S = _template_persons(what, crop_meta_p, n_p, track_id, frame_stream, trk_meta)
    if weight not in TEMPLATE_WEIGHTS:
        raise ValueError(f"{what}: weight must be one of {sorted(TEMPLATE_WEIGHTS)}, got {weight!r}")
    min_norm = float(min_norm)
    if min_norm != min_norm:
        raise ValueError(f"{what}: min_norm must be a number")
    e = embeddings
    if not (isinstance(e, torch.Tensor) and e.is_cuda and e.dtype == torch.float32 and e.dim() == 2 and e.shape[0] >= 1
            and (e.shape[1] == 1 or e.stride(1) == 1) and e.stride(0) >= e.shape[1]):
        raise ValueError(f"{what}: embeddings must be a float32 device tensor [F >= 1, D] with unit stride along D and "
                         f"a row stride of at least D")
    F, D = e.shape
    _gallery_dim(what, D)
    T = TRACK_SLOTS
    _check_dev(what, "person_face", person_face, torch.int32, (P,))
    _check_dev(what, "norms", norms, torch.float32, (F,))
    _check_dev(what, "n_f", n_f, torch.int32, (1,))
    _check_dev(what, "tmpl_owner", tmpl_owner, torch.int32, (S, T))
    _check_dev(what, "tmpl_sum", tmpl_sum, torch.int64, (S, T, D))
    _check_dev(what, "tmpl_n", tmpl_n, torch.int32, (S, T))
    _check_dev(what, "tmpl_ident", tmpl_ident, torch.int64, (S, T))
    _check_dev(what, "tmpl_score", tmpl_score, torch.float32, (S, T))
    if not (isinstance(queries, torch.Tensor) and queries.dim() == 2 and queries.shape[0] >= min(S * T, F)):
        raise ValueError(f"{what}: queries must be [Q >= min(S * {T}, F) = {min(S * T, F)}, D]")
    Q = queries.shape[0]
    _check_dev(what, "queries", queries, torch.float32, (Q, D))
    _check_dev(what, "dirty_rows", dirty_rows, torch.int32, (Q,))
    _check_dev(what, "n_dirty", n_dirty, torch.int32, (1,))
    _check_dev(what, "dirty_pos", dirty_pos, torch.int32, (S, T))
    check(lib().prpe_track_template_update(crop_meta_p.data_ptr(), n_p.data_ptr(), P, track_id.data_ptr(),
                                           person_face.data_ptr(), e.data_ptr(), e.stride(0), norms.data_ptr(),
                                           n_f.data_ptr(), F, D, frame_stream.data_ptr(), B, S, trk_meta.data_ptr(),
                                           TEMPLATE_WEIGHTS[weight], min_norm, tmpl_owner.data_ptr(),
                                           tmpl_sum.data_ptr(), tmpl_n.data_ptr(), tmpl_ident.data_ptr(),
                                           tmpl_score.data_ptr(), dirty_rows.data_ptr(), n_dirty.data_ptr(),
                                           dirty_pos.data_ptr(), queries.data_ptr(), Q, _stream()), what)
    return dirty_rows, n_dirty, dirty_pos, queries


def track_template_assign(crop_meta_p, n_p, track_id, frame_stream, trk_meta, ident, score, n_dirty, dirty_rows,
                          dirty_pos, *, tmpl_n, tmpl_ident, tmpl_score, template_ident, template_score, template_faces):
    """The gallery's answer for the templates that changed, back into the state and out to the persons
    (prpe_track_template_assign, include/prpe.h): ident [Q] int64 and score [Q] are the search's
    result on ``queries`` of ``track_template_update``, whose n_dirty, dirty_rows and dirty_pos come
    along; tmpl_ident and tmpl_score take them at the listed slots. Per person slot: template_ident
    [P] int64, template_score [P] and template_faces [P] int32, (-1, -inf, 0) for a person without
    a live track. No host read."""
    what = "prpe_track_template_assign"
    P, B, S = _template_persons(what, crop_meta_p, n_p, track_id, frame_stream, trk_meta)
    if not (isinstance(ident, torch.Tensor) and ident.dim() == 1 and ident.shape[0] >= 1):
        raise ValueError(f"{what}: ident must be [Q >= 1]")
    Q, T = ident.shape[0], TRACK_SLOTS
    _check_dev(what, "ident", ident, torch.int64, (Q,))
    _check_dev(what, "score", score, torch.float32, (Q,))
    _check_dev(what, "n_dirty", n_dirty, torch.int32, (1,))
    _check_dev(what, "dirty_rows", dirty_rows, torch.int32, (Q,))
    _check_dev(what, "dirty_pos", dirty_pos, torch.int32, (S, T))
    _check_dev(what, "tmpl_n", tmpl_n, torch.int32, (S, T))
    _check_dev(what, "tmpl_ident", tmpl_ident, torch.int64, (S, T))
    _check_dev(what, "tmpl_score", tmpl_score, torch.float32, (S, T))
    _check_dev(what, "template_ident", template_ident, torch.int64, (P,))
    _check_dev(what, "template_score", template_score, torch.float32, (P,))
    _check_dev(what, "template_faces", template_faces, torch.int32, (P,))
    check(lib().prpe_track_template_assign(crop_meta_p.data_ptr(), n_p.data_ptr(), P, track_id.data_ptr(),
                                           frame_stream.data_ptr(), B, S, trk_meta.data_ptr(), ident.data_ptr(),
                                           score.data_ptr(), n_dirty.data_ptr(), dirty_rows.data_ptr(),
                                           dirty_pos.data_ptr(), Q, tmpl_n.data_ptr(), tmpl_ident.data_ptr(),
                                           tmpl_score.data_ptr(), template_ident.data_ptr(), template_score.data_ptr(),
                                           template_faces.data_ptr(), _stream()), what)
    return template_ident, template_score, template_faces


# ------------------------------------------------------------------ face identification (csrc/gallery.hip)
GALLERY_MAX_K = 8
GALLERY_MAX_DIM = 512
GALLERY_STEP_ROWS = 64               # gallery rows a workgroup takes per step: 4 waves x one 16-row MFMA tile


def gallery_plan(Q, G):
    """(query block width, query blocks, rows per chunk, chunks) of a search of ``Q`` queries over
    ``G`` rows: the host-side launch plan of prpe_gallery_topk restated (csrc/gallery.hip,
    ``gallery_plan``). The results never depend on it; tests use it to aim at chunk boundaries."""
    qb = 16 if Q <= 16 else 64
    nqb = -(-Q // qb)
    tiles = -(-G // GALLERY_STEP_ROWS)
    target = 1024 if Q <= 16 else max(512 // nqb, 1)
    tpc = -(-tiles // target)
    return qb, nqb, tpc * GALLERY_STEP_ROWS, -(-tiles // tpc)


def _gallery_dim(what, D):
    if D % 32 or not 32 <= D <= GALLERY_MAX_DIM:
        raise ValueError(f"{what}: the embedding width must be a multiple of 32 in [32, {GALLERY_MAX_DIM}], got {D}")


def gallery_enrol(x, gallery, norms, row0=0):
    """L2-normalise the rows of ``x`` [n, D] (float32 device, contiguous) into ``gallery`` [capacity, D]
    at rows row0 .. row0 + n, their norms into ``norms`` [capacity] (prpe_gallery_enrol,
    include/prpe.h). No other row is touched; nothing is read back."""
    what = "prpe_gallery_enrol"
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and isinstance(gallery, torch.Tensor) and gallery.dim() == 2):
        raise ValueError(f"{what}: x must be [n, D] and gallery [capacity, D]")
    n, D = x.shape
    capacity = gallery.shape[0]
    _gallery_dim(what, D)
    _check_dev(what, "x", x, torch.float32, (n, D))
    _check_dev(what, "gallery", gallery, torch.float32, (capacity, D))
    _check_dev(what, "norms", norms, torch.float32, (capacity,))
    row0 = int(row0)
    if n < 1 or row0 < 0 or row0 + n > capacity or gallery.data_ptr() % 16:
        raise ValueError(f"{what}: rows [{row0}, {row0 + n}) do not fit a 16-byte aligned gallery of {capacity} rows")
    check(lib().prpe_gallery_enrol(x.data_ptr(), D, n, D, gallery.data_ptr(), norms.data_ptr(), capacity, row0,
                                   _stream()), what)
    return gallery, norms


def gallery_topk(queries, gallery, G, k, *, scores, rows, valid=None, labels=None, threshold=0.0, ident=None,
                 workspace=None):
    """Cosine top-k of ``queries`` [Q, D] against rows [0, G) of ``gallery`` [capacity, D]
    (prpe_gallery_topk, include/prpe.h): fills scores [Q, k] float32 and rows [Q, k] int32, ordered
    by score descending then row ascending; (-inf, -1) past the number of candidates. ``valid``
    [>= G] uint8: 0 skips the row. With ``labels`` [>= G] int64 and ``ident`` [Q] int64:
    ident[q] = labels[rows[q, 0]] when scores[q, 0] >= threshold, else -1. ``workspace``: a uint8
    device tensor of at least prpe_gallery_topk_workspace_bytes(Q, G, k) bytes (allocated here when
    None). No host read."""
    return _gallery_topk("prpe_gallery_topk", queries, gallery, G, k, scores, rows, valid, labels, threshold, ident,
                         workspace, None, False)


def _gallery_topk(what, queries, gallery, G, k, scores, rows, valid, labels, threshold, ident, workspace, route, wide):
    if not (isinstance(queries, torch.Tensor) and queries.dim() == 2 and isinstance(gallery, torch.Tensor) and
            gallery.dim() == 2):
        raise ValueError(f"{what}: queries must be [Q, D] and gallery [capacity, D]")
    Q, D = queries.shape
    capacity = gallery.shape[0]
    G, k = int(G), int(k)
    _gallery_dim(what, D)
    if Q < 1 or not 1 <= G <= capacity or not 1 <= k <= GALLERY_MAX_K:
        raise ValueError(f"{what}: Q = {Q}, G = {G} of {capacity} rows, k = {k} (1..{GALLERY_MAX_K})")
    _check_dev(what, "queries", queries, torch.float32, (Q, D))
    _check_dev(what, "gallery", gallery, torch.float32, (capacity, D))
    _check_dev(what, "scores", scores, torch.float32, (Q, k))
    _check_dev(what, "rows", rows, torch.int32, (Q, k))
    if valid is not None:
        _check_dev(what, "valid", valid, torch.uint8, min_numel=G)
    if (labels is None) != (ident is None):
        raise ValueError(f"{what}: labels and ident go together")
    if labels is not None:
        _check_dev(what, "labels", labels, torch.int64, min_numel=G)
        _check_dev(what, "ident", ident, torch.int64, (Q,))
    if route is not None:
        _check_dev(what, "route", route, torch.uint8, (Q,))
    nbytes = getattr(lib(), what + "_workspace_bytes")(Q, G, k)
    if nbytes < 0:
        raise ValueError(f"{what}: {what}_workspace_bytes({Q}, {G}, {k}) failed")
    if workspace is None:
        workspace = torch.empty(nbytes, device=queries.device, dtype=torch.uint8)
    _check_dev(what, "workspace", workspace, torch.uint8, min_numel=nbytes)
    if gallery.data_ptr() % 16 or workspace.data_ptr() % 256:
        raise ValueError(f"{what}: the gallery must be 16-byte and the workspace 256-byte aligned")
    head = (queries.data_ptr(), D, Q, D, gallery.data_ptr(), G, _ptr(valid), k, scores.data_ptr(), rows.data_ptr(),
            _ptr(labels), float(threshold), _ptr(ident))
    tail = (workspace.data_ptr(), workspace.numel(), _stream())
    if wide:
        check(lib().prpe_gallery_topk_wide(*head, _ptr(route), *tail), what)
    else:
        check(lib().prpe_gallery_topk(*head, *tail), what)
    return scores, rows


GALLERY_WIDE_QB = 64                 # queries a filter workgroup holds in LDS
GALLERY_WIDE_L = 8                   # entries of a (chunk, query) list of the filter
GALLERY_WIDE_C = 64                  # candidates the exact re-score takes per query
GALLERY_ROUTES = ("exact", "wide", "auto")
# "auto" takes the wide route for at least this many queries against at least this many rows: at
# 1 M rows the wide route's slowest run beat the exact route's fastest from Q = 64 on (the smallest
# such measured Q), at 10 000 rows it lost at every measured Q but one, so no Q serves both sizes
# and "auto" stays on the exact route below the larger measured size
GALLERY_WIDE_MIN_Q = 64
GALLERY_WIDE_MIN_G = 1_000_000


def gallery_wide_eps(D):
    """PRPE_GALLERY_WIDE_EPS(D) of include/prpe.h: the proven bound on |coarse - exact| for unit or
    zero rows (2^-7 + 2^-16 + D 2^-22)."""
    return 2.0 ** -7 + 2.0 ** -16 + D * 2.0 ** -22


def gallery_wide_plan(Q, G):
    """(query blocks, rows per chunk, chunks) of the wide route's filter: ``wide_plan`` of
    csrc/gallery_wide.hip restated. The results never depend on it; tests use it to aim at chunk
    boundaries and to restate the certificate."""
    nqb = -(-Q // GALLERY_WIDE_QB)
    tiles = -(-G // GALLERY_STEP_ROWS)
    target = max(512 // nqb, 64)
    tpc = -(-tiles // target)
    return nqb, tpc * GALLERY_STEP_ROWS, -(-tiles // tpc)


def gallery_route(route, Q, G):
    """The route a search of ``Q`` queries over ``G`` rows takes under the setting ``route``:
    "exact" or "wide"."""
    if route not in GALLERY_ROUTES:
        raise ValueError(f"gallery route must be one of {GALLERY_ROUTES}, got {route!r}")
    if route == "auto":
        return "wide" if Q >= GALLERY_WIDE_MIN_Q and G >= GALLERY_WIDE_MIN_G else "exact"
    return route


def gallery_topk_wide(queries, gallery, G, k, *, scores, rows, valid=None, labels=None, threshold=0.0, ident=None,
                      route=None, workspace=None):
    """``gallery_topk`` for many queries per call (prpe_gallery_topk_wide, include/prpe.h): the same
    arguments, the same checks and the same bits in scores, rows and ident. A bf16 filter finds a
    provably sufficient candidate set per query, the candidates are scored exactly, and a query the
    filter cannot certify is finished by the exact kernels on the device. ``route`` (optional)
    [Q] uint8 receives 0 for a certified query and 1 for one the exact kernels finished.
    ``workspace``: at least prpe_gallery_topk_wide_workspace_bytes(Q, G, k) bytes. The gallery rows
    must be ``gallery_enrol``'s output. No host read."""
    return _gallery_topk("prpe_gallery_topk_wide", queries, gallery, G, k, scores, rows, valid, labels, threshold,
                         ident, workspace, route, True)


# ------------------------------------------------------------------ face verification (csrc/pairhist.hip)
PAIR_HIST_TILE = 128                 # rows and columns of the score tile a workgroup takes
PAIR_HIST_BINS = (256, 512, 1024, 2048, 4096)
PAIR_HIST_MAX_ROWS = 1 << 24


def _pair_rows(what, name, t, D):
    """``t`` [n, D] float32 on the device, unit column stride, row stride >= D and a multiple of 4,
    16-byte aligned; returns (n, row stride)."""
    ok = (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and
          t.shape[1] == D and 1 <= t.shape[0] <= PAIR_HIST_MAX_ROWS)
    if ok:
        ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), D)
        ok = t.stride(1) == 1 and ld >= D and ld % 4 == 0 and t.data_ptr() % 16 == 0
    if not ok:
        got = (type(t).__name__ if not isinstance(t, torch.Tensor) else
               f"{t.dtype} {list(t.shape)} strides {list(t.stride())} on {t.device}")
        raise ValueError(f"{what}: {name} must be a float32 device tensor [1..2^24, {D}] with unit column stride, a "
                         f"row stride >= {D} that is a multiple of 4 and a 16-byte aligned start, got {got}")
    return t.shape[0], ld


def pair_hist(a, a_labels, b=None, b_labels=None, *, nbins, hist, skipped, a_valid=None, b_valid=None):
    """Scores of all pairs of already normalised rows (``gallery_enrol``'s output), binned
    (prpe_pair_hist, include/prpe.h). ``b`` None: the pairs i < j of ``a`` [M, D]; else all pairs of
    ``a`` and ``b`` [N, D]. Labels int64 [M] / [N]; a row with a negative label or a zero byte in
    ``a_valid`` / ``b_valid`` (uint8, optional) takes part in no pair. ``hist`` int64 [2, nbins]
    (row 0 genuine, row 1 impostor) and ``skipped`` int64 [1] (pairs whose score is not finite) are
    ADDED to: the caller zeroes them. No host read."""
    what = "prpe_pair_hist"
    if not (isinstance(a, torch.Tensor) and a.dim() == 2):
        raise ValueError(f"{what}: a must be [M, D]")
    D = a.shape[1]
    _gallery_dim(what, D)
    nbins = int(nbins)
    if nbins not in PAIR_HIST_BINS:
        raise ValueError(f"{what}: nbins must be one of {PAIR_HIST_BINS}, got {nbins}")
    M, lda = _pair_rows(what, "a", a, D)
    _check_dev(what, "a_labels", a_labels, torch.int64, (M,))
    if a_valid is not None:
        _check_dev(what, "a_valid", a_valid, torch.uint8, (M,))
    N, ldb = 0, 0
    if b is None:
        if b_labels is not None or b_valid is not None:
            raise ValueError(f"{what}: b_labels and b_valid need b")
    else:
        N, ldb = _pair_rows(what, "b", b, D)
        _check_dev(what, "b_labels", b_labels, torch.int64, (N,))
        if b_valid is not None:
            _check_dev(what, "b_valid", b_valid, torch.uint8, (N,))
    _check_dev(what, "hist", hist, torch.int64, (2, nbins))
    _check_dev(what, "skipped", skipped, torch.int64, (1,))
    check(lib().prpe_pair_hist(a.data_ptr(), lda, M, a_labels.data_ptr(), _ptr(a_valid), _ptr(b), ldb, N,
                               _ptr(b_labels), _ptr(b_valid), D, nbins, hist.data_ptr(), skipped.data_ptr(),
                               _stream()), what)
    return hist, skipped


# ------------------------------------------------------------------ face clustering (csrc/facecluster.hip)
def face_cluster_workspace_bytes(N):
    """Bytes of the workspace ``pair_link`` and ``cluster_finish`` share for ``N`` rows
    (prpe_face_cluster_workspace_bytes: best [N] uint64, parent [N] int32)."""
    nbytes = lib().prpe_face_cluster_workspace_bytes(int(N))
    if nbytes < 0:
        raise ValueError(f"prpe_face_cluster_workspace_bytes({N}) failed")
    return nbytes


def _cluster_rows(what, a, valid):
    if not (isinstance(a, torch.Tensor) and a.dim() == 2):
        raise ValueError(f"{what}: a must be [N, D]")
    D = a.shape[1]
    _gallery_dim(what, D)
    N, lda = _pair_rows(what, "a", a, D)
    if valid is not None:
        _check_dev(what, "valid", valid, torch.uint8, (N,))
    return N, D, lda


def _cluster_threshold(what, threshold, min_samples=1):
    threshold, min_samples = float(threshold), int(min_samples)
    if not math.isfinite(threshold) or min_samples < 1:
        raise ValueError(f"{what}: the threshold must be finite and min_samples >= 1, got {threshold}, {min_samples}")
    return threshold, min_samples


def _cluster_workspace(what, workspace, N):
    _check_dev(what, "workspace", workspace, torch.uint8, min_numel=face_cluster_workspace_bytes(N))
    if workspace.data_ptr() % 256:
        raise ValueError(f"{what}: the workspace must be 256-byte aligned")


def pair_degree(a, threshold, *, degree, valid=None):
    """Pass 1 of the clustering (prpe_pair_degree, include/prpe.h): ``degree`` [N] int32 is
    overwritten with every row's number of neighbours among the already normalised rows ``a``
    [N, D] at ``threshold``. ``valid`` [N] uint8, optional: 0 leaves the row out. No host read."""
    what = "prpe_pair_degree"
    N, D, lda = _cluster_rows(what, a, valid)
    threshold, _ = _cluster_threshold(what, threshold)
    _check_dev(what, "degree", degree, torch.int32, (N,))
    check(lib().prpe_pair_degree(a.data_ptr(), lda, N, _ptr(valid), D, threshold, degree.data_ptr(), _stream()), what)
    return degree


def pair_link(a, threshold, min_samples, *, degree, workspace, valid=None):
    """Pass 2 (prpe_pair_link): with ``degree`` from ``pair_degree`` at the same threshold, links
    the core rows of a cluster under one root and records every other row's best core neighbour,
    in ``workspace`` (uint8, >= face_cluster_workspace_bytes(N), 256-byte aligned). No host read."""
    what = "prpe_pair_link"
    N, D, lda = _cluster_rows(what, a, valid)
    threshold, min_samples = _cluster_threshold(what, threshold, min_samples)
    _check_dev(what, "degree", degree, torch.int32, (N,))
    _cluster_workspace(what, workspace, N)
    check(lib().prpe_pair_link(a.data_ptr(), lda, N, _ptr(valid), D, threshold, min_samples, degree.data_ptr(),
                               workspace.data_ptr(), workspace.numel(), _stream()), what)
    return workspace


def cluster_finish(N, min_samples, *, degree, workspace, root, kind, cluster, n_clusters, sizes, valid=None):
    """Flatten, classify and compact (prpe_cluster_finish): fills root [N] int32, kind [N] uint8
    (0 left out, 1 noise, 2 border, 3 core), cluster [N] int32, n_clusters [1] int32 and
    sizes[0 .. min(C, max_clusters)) with max_clusters = sizes.numel(). No host read."""
    what = "prpe_cluster_finish"
    N = int(N)
    _, min_samples = _cluster_threshold(what, 0.0, min_samples)
    if not 1 <= N <= PAIR_HIST_MAX_ROWS:
        raise ValueError(f"{what}: N must lie in [1, 2^24], got {N}")
    if valid is not None:
        _check_dev(what, "valid", valid, torch.uint8, (N,))
    _check_dev(what, "degree", degree, torch.int32, (N,))
    _cluster_workspace(what, workspace, N)
    _check_dev(what, "root", root, torch.int32, (N,))
    _check_dev(what, "kind", kind, torch.uint8, (N,))
    _check_dev(what, "cluster", cluster, torch.int32, (N,))
    _check_dev(what, "n_clusters", n_clusters, torch.int32, (1,))
    _check_dev(what, "sizes", sizes, torch.int32, min_numel=1)
    if sizes.dim() != 1:
        raise ValueError(f"{what}: sizes must be [max_clusters]")
    check(lib().prpe_cluster_finish(N, _ptr(valid), min_samples, degree.data_ptr(), workspace.data_ptr(),
                                    workspace.numel(), root.data_ptr(), kind.data_ptr(), cluster.data_ptr(),
                                    n_clusters.data_ptr(), sizes.numel(), sizes.data_ptr(), _stream()), what)
    return root, kind, cluster, n_clusters, sizes


def cluster_centroids(a, *, cluster, n_clusters, sums, centroids):
    """Per-cluster fixed-point sums and centroids (prpe_cluster_centroids): sums [max_clusters, D]
    int64 and centroids [max_clusters, D] float32 (not normalised), rows [0, min(C, max_clusters))
    written, the others left as they are. No host read."""
    what = "prpe_cluster_centroids"
    N, D, lda = _cluster_rows(what, a, None)
    _check_dev(what, "cluster", cluster, torch.int32, (N,))
    _check_dev(what, "n_clusters", n_clusters, torch.int32, (1,))
    if not (isinstance(sums, torch.Tensor) and sums.dim() == 2 and sums.shape[0] >= 1):
        raise ValueError(f"{what}: sums must be [max_clusters >= 1, D]")
    max_clusters = sums.shape[0]
    _check_dev(what, "sums", sums, torch.int64, (max_clusters, D))
    _check_dev(what, "centroids", centroids, torch.float32, (max_clusters, D))
    check(lib().prpe_cluster_centroids(a.data_ptr(), lda, N, D, cluster.data_ptr(), n_clusters.data_ptr(), max_clusters,
                                       sums.data_ptr(), centroids.data_ptr(), _stream()), what)
    return sums, centroids


# ------------------------------------------------------------------ identification evaluation (csrc/identeval.hip)
IDENT_RANKS = 64                     # PRPE_IDENT_RANKS: rank_hist has IDENT_RANKS + 1 slots


def _ident_operands(what, a, a_labels, b, b_labels, a_valid, b_valid, b_row0):
    """The operand checks ``ident_best`` and ``ident_rank`` share; returns the leading arguments
    of the C call and M."""
    if not (isinstance(a, torch.Tensor) and a.dim() == 2):
        raise ValueError(f"{what}: a must be [M, D]")
    D = a.shape[1]
    _gallery_dim(what, D)
    M, lda = _pair_rows(what, "a", a, D)
    _check_dev(what, "a_labels", a_labels, torch.int64, (M,))
    if a_valid is not None:
        _check_dev(what, "a_valid", a_valid, torch.uint8, (M,))
    N, ldb, b_row0 = 0, 0, int(b_row0)
    if b is None:
        if b_labels is not None or b_valid is not None or b_row0 != 0:
            raise ValueError(f"{what}: b_labels, b_valid and b_row0 need b")
    else:
        N, ldb = _pair_rows(what, "b", b, D)
        _check_dev(what, "b_labels", b_labels, torch.int64, (N,))
        if b_valid is not None:
            _check_dev(what, "b_valid", b_valid, torch.uint8, (N,))
        if not 0 <= b_row0 <= 2 ** 31 - 1 - N:
            raise ValueError(f"{what}: b_row0 must lie in [0, 2^31 - 1 - N], got {b_row0}")
    return (a.data_ptr(), lda, M, a_labels.data_ptr(), _ptr(a_valid), _ptr(b), ldb, N, _ptr(b_labels), _ptr(b_valid),
            b_row0, D), M


def ident_best(a, a_labels, b=None, b_labels=None, *, mate_key, non_key, skipped, a_valid=None, b_valid=None,
               b_row0=0):
    """Pass 1 of the identification evaluation (prpe_ident_best, include/prpe.h): per probe row of
    ``a`` [M, D] the largest candidate key among the rows of ``b`` [N, D] with the probe's label
    (``mate_key``) and among the others (``non_key``), both int64 [M] holding the uint64 keys,
    raised by atomic maxima: the caller zeroes them. ``b`` None: leave-one-out on ``a``.
    ``b_row0``: the number of ``b``'s first row, for a gallery passed in several ranges. ``skipped``
    int64 [1] is ADDED the combinations whose score is not finite. Rows are already normalised
    (``gallery_enrol``'s output). No host read."""
    what = "prpe_ident_best"
    args, M = _ident_operands(what, a, a_labels, b, b_labels, a_valid, b_valid, b_row0)
    _check_dev(what, "mate_key", mate_key, torch.int64, (M,))
    _check_dev(what, "non_key", non_key, torch.int64, (M,))
    _check_dev(what, "skipped", skipped, torch.int64, (1,))
    check(lib().prpe_ident_best(*args, mate_key.data_ptr(), non_key.data_ptr(), skipped.data_ptr(), _stream()), what)
    return mate_key, non_key, skipped


def ident_rank(a, a_labels, b=None, b_labels=None, *, mate_key, rank_minus_1, a_valid=None, b_valid=None, b_row0=0):
    """Pass 2 (prpe_ident_rank): with ``mate_key`` of the whole gallery from ``ident_best``,
    ``rank_minus_1`` int32 [M] is ADDED the number of non-mate candidates ahead of each probe's best
    mate; the caller zeroes it. The operands are ``ident_best``'s. No host read."""
    what = "prpe_ident_rank"
    args, M = _ident_operands(what, a, a_labels, b, b_labels, a_valid, b_valid, b_row0)
    _check_dev(what, "mate_key", mate_key, torch.int64, (M,))
    _check_dev(what, "rank_minus_1", rank_minus_1, torch.int32, (M,))
    check(lib().prpe_ident_rank(*args, mate_key.data_ptr(), rank_minus_1.data_ptr(), _stream()), what)
    return rank_minus_1


def ident_finish(a_labels, *, mate_key, non_key, nbins, mate_score, mate_row, non_score, non_row, rank, hist, counts,
                 rank_minus_1=None, rank_hist=None, a_valid=None):
    """Decode and bin (prpe_ident_finish): writes mate_score / non_score float32 [M], mate_row /
    non_row / rank int32 [M]; ADDS the probes to ``hist`` int64 [3, nbins] (right label, wrong
    label, stranger named), ``rank_hist`` int64 [IDENT_RANKS + 1] and ``counts`` int64 [4] (mated,
    non-mated, left out, without any candidate): the caller zeroes these. ``rank_minus_1`` and
    ``rank_hist`` go together; without them ``rank`` is 1, 0 or -1 (above 1). No host read."""
    what = "prpe_ident_finish"
    if not (isinstance(a_labels, torch.Tensor) and a_labels.dim() == 1 and 1 <= a_labels.shape[0] <= PAIR_HIST_MAX_ROWS):
        raise ValueError(f"{what}: a_labels must be [1..2^24]")
    M = a_labels.shape[0]
    nbins = int(nbins)
    if nbins not in PAIR_HIST_BINS:
        raise ValueError(f"{what}: nbins must be one of {PAIR_HIST_BINS}, got {nbins}")
    _check_dev(what, "a_labels", a_labels, torch.int64, (M,))
    if a_valid is not None:
        _check_dev(what, "a_valid", a_valid, torch.uint8, (M,))
    _check_dev(what, "mate_key", mate_key, torch.int64, (M,))
    _check_dev(what, "non_key", non_key, torch.int64, (M,))
    if (rank_minus_1 is None) != (rank_hist is None):
        raise ValueError(f"{what}: rank_minus_1 and rank_hist go together")
    if rank_minus_1 is not None:
        _check_dev(what, "rank_minus_1", rank_minus_1, torch.int32, (M,))
        _check_dev(what, "rank_hist", rank_hist, torch.int64, (IDENT_RANKS + 1,))
    _check_dev(what, "mate_score", mate_score, torch.float32, (M,))
    _check_dev(what, "non_score", non_score, torch.float32, (M,))
    _check_dev(what, "mate_row", mate_row, torch.int32, (M,))
    _check_dev(what, "non_row", non_row, torch.int32, (M,))
    _check_dev(what, "rank", rank, torch.int32, (M,))
    _check_dev(what, "hist", hist, torch.int64, (3, nbins))
    _check_dev(what, "counts", counts, torch.int64, (4,))
    check(lib().prpe_ident_finish(M, a_labels.data_ptr(), _ptr(a_valid), mate_key.data_ptr(), non_key.data_ptr(),
                                  _ptr(rank_minus_1), nbins, mate_score.data_ptr(), mate_row.data_ptr(),
                                  non_score.data_ptr(), non_row.data_ptr(), rank.data_ptr(), hist.data_ptr(),
                                  _ptr(rank_hist), counts.data_ptr(), _stream()), what)
    return hist, rank_hist, counts
