"""The per-frame inference hot path on MI355X: every layer of the combined model runs as a
hand-written HIP kernel through the C ABI (prpe.ops -> libprpe.so). No torch compute op
is used on the data path; PyTorch only provides device buffers and the stream.

Layout: activations are NHWC float32 (channels contiguous => coalesced implicit-GEMM
reads); concat buffers are allocated once per concat and producers write straight into
their channel slice (no torch.cat copies); the detection head writes its per-level
outputs straight into one [B, 525, 65] buffer that the DFL decoder reads.

Exact algebraic rewrite of every "bilinear upsample -> conv3x3" pair (the three adapters
and the ViTPose decoder, 60 % of the reference FLOPs): conv3x3(U(x)) is evaluated as a
low-resolution 1x1 GEMM producing 9 per-tap maps, then one fused kernel interpolates and
sums the taps and applies BN/act (prpe_upconv3x3). Same function, fp32-rounding-level
differences, ~40x fewer executed FLOPs on those layers.

Reference structure mirrored function by function (see prpe.arch for citations).
"""
from __future__ import annotations

import os

import torch

from . import arch, ops
from ._lib import RES_POST, RES_PRE
from .nv12 import NV12Frames
from .pack import ConvPack, bn_affine, pack_conv, pack_matrix, pack_upconv_taps

YOLO_BN_EPS = 1e-3
BN_EPS = 1e-5


# Per-component conv precision (prpe_conv2d ``precision``): 2 = 3-plane bf16 split, exact fp32
# operands (6 MFMA terms); 3 = 2-plane fp16 split with power-of-2 scaling (3 terms, ~2^-21 per
# operand, below fp32's own accumulation error; needs a chunked input with a tracked max|x|,
# else the conv runs precision 2); 0 = 2-plane bf16 split (3 terms, ~2^-17); 4 = ONE scaled
# fp16 plane (1 term, ~2^-12 per operand; per-frame max|x| tracked through the component, else
# the conv runs precision 0). "auto" keeps fp32-faithful products where errors are amplified
# most (measured, DESIGN.md "Precision"): the ResNet-50 trunk every head consumes, and the small
# YOLO net whose DFL box decode multiplies logit errors by the stride; the large adapters and
# the ViT run the bf16 3-term split; the AdaFace branch (adapter + IR-50), whose embedding is
# least sensitive to operand rounding (precision study: 1.8e-4 against the 1e-3 bar), runs one
# fp16 term (round 4). PRPE_ADAFACE_PREC=0 or 3 restores a 3-term split there (A/B runs); it is
# read when an Engine is built (auto_policy), not at import.
AUTO_POLICY = {"trunk": 3, "yolo_adapter": 0, "yolo_net": 2, "vit": 0, "adaface": 4}
ADAFACE_PRECS = (0, 3, 4)


def auto_policy() -> dict:
    """AUTO_POLICY with the PRPE_ADAFACE_PREC override of the environment as it is now."""
    pol = dict(AUTO_POLICY)
    env = os.environ.get("PRPE_ADAFACE_PREC")
    if env is not None:
        try:
            v = int(env)
        except ValueError:
            v = None
        if v not in ADAFACE_PRECS:
            raise ValueError(f"PRPE_ADAFACE_PREC={env!r}: expected one of {ADAFACE_PRECS}")
        pol["adaface"] = v
    return pol


F16_PRECS = (3, 4)                  # precisions that read / keep per-frame max|x| slots
AMAX_CHUNK = 1 << 16                # floats per chunk of a component's max|y| slot pool
# PRPE_PLANES=0 keeps every activation in fp32 (A/B runs of the planes-format handoff)
PLANES_ON = os.environ.get("PRPE_PLANES", "1") != "0"
# 3x3/1 convs with Co <= 4 (the last conv of the YOLO and ViTPose adapters) as the tap rewrite
# at unit scale: one read of the input by a 1x1 GEMM to the 9*Co tap maps, then a shifted tap
# sum (prpe_upconv3x3 with an identity resample). PRPE_SMALLCO_TAPS=0 keeps the direct conv.
SMALLCO_TAPS = os.environ.get("PRPE_SMALLCO_TAPS", "1") != "0"
# ... and where the producer of that conv's input is a haloed-tile 3x3 conv (ViTPose adapter.7 ->
# .10), the tap GEMM runs in the producer's epilogue (prpe_conv_desc.w2): the 128-channel map
# never reaches HBM. PRPE_TAPS_FUSE=0 runs the two convs separately.
TAPS_FUSE = os.environ.get("PRPE_TAPS_FUSE", "1") != "0"
# ResNet-50 identity blocks (1.1, 1.2) as ONE fused launch each (prpe_bottleneck: t1 / t2
# only in LDS). PRPE_BNECK_FUSE=0 runs the three convs separately. Block 1.0 (conv3 + the
# downsample projection as one dual GEMM) likewise; PRPE_BNECK_PROJ=0 keeps it unfused.
BNECK_FUSE = os.environ.get("PRPE_BNECK_FUSE", "1") != "0"
BNECK_PROJ = os.environ.get("PRPE_BNECK_PROJ", "1") != "0"
# ... and layer2's identity blocks (2.1-2.3, inner width 128, one 160-KB workgroup per CU);
# PRPE_BNECK_L2=0 keeps them unfused
BNECK_L2 = os.environ.get("PRPE_BNECK_L2", "1") != "0"
# stem conv + max-pool as ONE launch (prpe_stem_maxpool: the [B, 320, 320, 64] stem map stays in
# LDS); PRPE_STEM_POOL=0 runs prpe_conv2d + prpe_maxpool
STEM_POOL = os.environ.get("PRPE_STEM_POOL", "1") != "0"
# ViTPose patch embedding (16x16/16 pad 2, 3 -> 768) as a chunked 16x1 conv over an overlapping view
# of a zero-bordered NHWC4 copy of the crops, as the stem (Engine.vit_pix4); PRPE_VIT_PATCH_VIEW=0
# runs the plain 16x16 conv on the 3-channel crops (the gather-bound small-Ci kernel)
PATCH_VIEW = os.environ.get("PRPE_VIT_PATCH_VIEW", "1") != "0"
# the unfused trunk blocks' 3x3 conv2 over a zero-bordered copy of its input, unpadded (no tap
# masks: conv_wave's pixel-contiguous A loads; Engine.bordered); PRPE_T1_BORDER=0 runs it with
# pad 1 on the plain conv1 output
T1_BORDER = os.environ.get("PRPE_T1_BORDER", "1") != "0"


class Act:
    """An activation as one layer hands it to the next: the device tensor (logical NHWC view) and
    what the engine knows about it. A view of ``t`` is a new tensor with none of this: where the
    metadata holds for the view too, the code builds a new Act there and says why."""
    __slots__ = ("t", "amax", "planes", "pooled", "epoch", "pix4")

    def __init__(self, t, amax=None, planes=False, pooled=False, epoch=None, pix4=None):
        self.t = t              # the device tensor
        self.amax = amax        # [N] device slots bounding max|t[n]| (precision 3/4 operand scale), or None
        self.planes = planes    # t holds bf16 hi/lo planes (include/prpe.h), not fp32
        self.pooled = pooled    # the stem launch already max-pooled
        self.epoch = epoch      # (component, n): amax is valid while the component's pool epoch is n
        self.pix4 = pix4        # the zero-bordered NHWC4 buffer t is the interior of, or None


def _act(x) -> Act:
    """``x`` as an Act: a bare tensor (frames, pixel_values, a slice of a concat buffer) carries no
    metadata."""
    return x if isinstance(x, Act) else Act(x)


class _Prec:
    """Component scope: its precision from the policy and, at precision 3, its own max|y| slot
    pool (zeroed on entry, on the current stream)."""

    def __init__(self, eng, comp):
        self.e, self.c = eng, comp

    def __enter__(self):
        self.saved = (self.e.precision, self.e._amax_scope)
        self.e.precision = self.e.policy.get(self.c, self.saved[0])
        if self.e.precision in F16_PRECS:
            self.e._amax_begin(self.c)

    def __exit__(self, *a):
        self.e.precision, scope = self.saved
        self.e._amax_scope = scope


class Engine:
    """precision: "auto" (AUTO_POLICY), an int 0/1/2 for every conv, or a policy dict."""

    def __init__(self, state_dict: dict, device="cuda", precision="auto"):
        self.sd = state_dict
        self.device = torch.device(device)
        if precision == "auto":
            self.policy = auto_policy()
        elif isinstance(precision, dict):
            self.policy = dict(auto_policy(), **precision)
        else:
            self.policy = {k: int(precision) for k in AUTO_POLICY}
        self.precision = 0
        self._packs: dict[str, ConvPack] = {}
        self._aux: dict[str, torch.Tensor] = {}
        self.watch: set[str] = set()      # pack names whose launches get HIP-event timing
        self.events: dict[str, list] = {}
        self.up_events: dict[str, list] = {}   # upconv launches (tools/layer_profile.py), when watched
        # per-component device pools of per-frame max|y| slots (precision 3): comp -> [chunk
        # tensors, cursor (chunk index, offset)]
        self._amax_pools: dict[str, list] = {}
        self._amax_scope = None
        self._amax_epoch: dict[str, int] = {}   # comp -> number of times its pool was zeroed

    def prec(self, comp):
        return _Prec(self, comp)

    # ------------------------------------------------------------------ helpers
    def empty(self, *shape):
        return torch.empty(*shape, device=self.device, dtype=torch.float32)

    def _batch_buf(self, kind, B, shape):
        """The zeroed scratch buffer [B, *shape] of ``kind``, allocated once per shape (callers
        only ever write its interior, so its border stays zero). A new batch size drops the
        kind's buffers of every other batch size: one batch size at a time."""
        key = (kind, B, *shape)
        t = self._aux.get(key)
        if t is None:
            for k in [k for k in self._aux if isinstance(k, tuple) and k[0] == kind and k[1] != B]:
                del self._aux[k]
            t = torch.zeros(B, *shape, device=self.device, dtype=torch.float32)
            self._aux[key] = t
        return t

    def bordered(self, B, H, W, C):
        """A [B, H+2, W+2, C] buffer whose one-pixel border is zero: the input of an unpadded
        3x3 conv."""
        return self._batch_buf("bordered", B, (H + 2, W + 2, C))

    def _timed(self, watch, events, key, rec, launch):
        """Run ``launch()``; when ``watch`` is in ``self.watch``, between two HIP events, and
        append (e0, e1, *rec) to ``events[key]`` (bench roofline, tools/layer_profile.py)."""
        if watch not in self.watch:
            return launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        events.setdefault(key, []).append((e0, e1, *rec))

    def dev(self, key, fn=None):
        t = self._aux.get(key)
        if t is None:
            v = self.sd[key] if fn is None else fn()
            t = v.float().contiguous().to(self.device)
            self._aux[key] = t
        return t

    def pk(self, name, wkey, stride=1, pad=0, bn=None, eps=BN_EPS, bias_key=None, act="none", prelu=None,
           in_bn=None, in_eps=BN_EPS) -> ConvPack:
        p = self._packs.get(name)
        if p is None:
            sd = self.sd
            cb = sd[bias_key] if bias_key else None
            if bn is not None:
                scale, bias = bn_affine(sd, bn, eps, cb)
            else:
                scale, bias = None, cb
            in_s = in_b = None
            if in_bn is not None:
                in_s, in_b = bn_affine(sd, in_bn, in_eps)
            slope = sd[prelu] if prelu else None
            p = pack_conv(name, sd[wkey], stride, pad, self.device, scale=scale, bias=bias, slope=slope,
                          in_scale=in_s, in_bias=in_b, act=act)
            self._packs[name] = p
        return p

    # ---- max|y| tracking: every conv output of a precision-3 component gets an [N] array of
    # per-row-group device slots (N = the conv's leading dim: frames, or tokens for the ViT's
    # [B*L, 1, 1, D] linears) its epilogue raises to max|y[n]|; a precision-3 consumer reads slot
    # n to pick row group n's activation scale, so a frame's arithmetic never depends on its
    # batch-mates (or on the shard it lands in). Each component scope (Engine.prec) owns a pool
    # of chunks, zeroed on entry on the current stream (the heads run on their own streams) and
    # grown by whole chunks on first use, so any batch and any number of convs fit.
    def _amax_begin(self, comp: str):
        pool = self._amax_pools.get(comp)
        if pool is None:
            pool = self._amax_pools[comp] = [[], 0, 0]
        for t in pool[0]:
            t.zero_()
        pool[1] = pool[2] = 0
        self._amax_scope = comp
        self._amax_epoch[comp] = self._amax_epoch.get(comp, 0) + 1

    def amax_slot(self, n: int):
        """[n] zeroed slots from the current precision-3 component's pool."""
        if self._amax_scope is None:
            raise RuntimeError("max|y| slots requested outside a precision-3 component scope (Engine.prec)")
        pool = self._amax_pools[self._amax_scope]
        chunks, ci, off = pool
        if ci < len(chunks) and off + n > chunks[ci].numel():
            ci, off = ci + 1, 0
        if ci == len(chunks):
            chunks.append(torch.zeros(max(AMAX_CHUNK, n), device=self.device, dtype=torch.float32))
        elif chunks[ci].numel() - off < n:
            # a chunk made for a smaller batch (chunks past the cursor are not handed out in this
            # scope yet): a bigger one takes its place, zeroed like every chunk of the pool
            chunks[ci] = torch.zeros(max(AMAX_CHUNK, n), device=self.device, dtype=torch.float32)
        t = chunks[ci][off:off + n]
        pool[1], pool[2] = ci, off + n
        return t

    @staticmethod
    def _vec4(t):
        """16-B vector rows (the precision-3 kernels' epilogue needs them for y and the residual)."""
        return t is None or (t.stride(3) == 1 and t.shape[3] % 4 == 0 and t.data_ptr() % 16 == 0 and
                             all(st % 4 == 0 for st in t.stride()[:3]))

    @staticmethod
    def _f16_ok(x, p: ConvPack, out, res=None, prologue=False):
        """``prologue``: an input-side affine is allowed (precision 4 bounds it in-kernel)."""
        chunked = p.k_order == 1 or (p.kh * p.kw == 1 and p.ci % 32 == 0)
        # (a planes-format input is read by precision 0 only: its consumer drops to 0 as well)
        return (chunked and (prologue or p.in_scale is None) and x.t.stride(3) == 1 and x.t.data_ptr() % 16 == 0 and
                Engine._vec4(out) and Engine._vec4(res) and x.amax is not None and not x.planes)

    def pk_dual(self, q) -> ConvPack:
        """Bottleneck ``q`` (block 0 of a stage): relu(bn3(conv3(o)) + bn_ds(downsample(x))) as
        one 1x1 GEMM over [o | x_sub] with each BN scale folded into its weight rows
        (W' = [s3 W3 | sd Wd], bias b3 + bd; torchvision Bottleneck.forward)."""
        name = q + ".conv3+downsample"
        p = self._packs.get(name)
        if p is None:
            sd = self.sd
            w3 = sd[q + ".conv3.weight"].float().flatten(1)
            wd = sd[q + ".downsample.0.weight"].float().flatten(1)
            s3, b3 = bn_affine(sd, q + ".bn3", BN_EPS)
            sdn, bd = bn_affine(sd, q + ".downsample.1", BN_EPS)
            w = torch.cat([w3 * s3[:, None], wd * sdn[:, None]], 1)
            p = pack_matrix(name, w, 1, 1, w.shape[1], 1, 0, self.device, bias=b3 + bd, act="relu")
            self._packs[name] = p
        return p

    def conv(self, x, p: ConvPack, out=None, res=None, res_mode=0, act=None, x2=None, planes_out=False, w2=None,
             y2=None, prec=None, track=True, **stage2):
        """``x``, ``res``: an Act or a bare tensor. ``out``: the caller's view to write (a tensor,
        or an Act, which is then the one returned). Returns the output as an Act.
        ``x2``: second 1x1 input on the output grid, an Act (dual-input GEMM, see prpe.h).
        ``planes_out``: the only consumer is a precision-0 wave-row conv: write the planes format.
        ``w2``/``y2``: epilogue 1x1 GEMM into y2 (prpe.h); ``out`` is then not written;
        ``stage2``: its second stage (w3, scale2, bias2, act2; prpe.h).
        ``prec``: this conv's precision instead of the component's (Engine.feat_prec).
        ``track``: raise the output's per-frame max|y| slots in a precision-3/4 component (off for
        an output no conv consumes, e.g. the IR-50 output layer's split-K GEMM)."""
        x, res = _act(x), res.t if isinstance(res, Act) else res
        if x.epoch is not None and self._amax_epoch.get(x.epoch[0]) != x.epoch[1]:
            # the component that wrote x's max|x| slots has re-zeroed its pool since (a later trunk
            # call): the slots now bound some other tensor, so x is read as one without any (a
            # precision-4 head would otherwise scale by them, as feat_prec's precision 3 would)
            x = Act(x.t, planes=x.planes)
        B, H, W, _ = x.t.shape
        Ho = (H + 2 * p.pad - p.kh) // p.stride + 1
        Wo = (W + 2 * p.pad - p.kw) // p.stride + 1
        out = _act(self.empty(B, Ho, Wo, p.co) if out is None else out)
        prec = self.precision if prec is None else prec
        if prec == 3 and (not self._f16_ok(x, p, out.t, res) or (x2 is not None and x2.amax is None)):
            prec = 2
        if prec == 4 and (not self._f16_ok(x, p, out.t, res, prologue=True) or x2 is not None):
            prec = 0
        xa = x.amax if prec in F16_PRECS else None
        ya = self.amax_slot(B) if self.precision in F16_PRECS and w2 is None and track else None
        if x.planes and prec != 0:
            raise RuntimeError(f"{p.name}: planes-format input needs precision 0, got {prec}")
        # planes output only where the component itself runs precision 0 (as upconv(): inside a
        # precision-3/4 scope a conv that fell back to 0 keeps fp32 output for its f16 consumers)
        y_planes = (PLANES_ON and planes_out and prec == 0 and self.precision == 0 and p.co % 8 == 0 and
                    out.t.is_contiguous())
        kw = dict(res=res, res_mode=res_mode, act=act, precision=prec, tile=p.tile, x_amax=xa, y_amax=ya,
                  x_planes=x.planes, y_planes=y_planes, w2=w2, y2=y2, **stage2)
        if x2 is not None:
            kw.update(x2=x2.t, x2_amax=x2.amax if prec == 3 else None)
        self._timed(p.name, self.events, p.name, (B * Ho * Wo, p, prec, x.t.numel()),
                    lambda: ops.conv2d(x.t, p, out.t, **kw))
        out.amax, out.planes = ya, y_planes
        return out

    def upconv(self, name, x, wkey, size, align_corners, bn=None, bias_key=None, act="none", prelu=None, out=None,
               planes=False, z=None):
        """conv3x3(pad 1)(bilinear_upsample(x, size)) [+BN] [+act] via the tap rewrite.
        ``planes``: the only consumer is a precision-0 conv, so write the planes format (the
        consumer's two-plane split done once here; include/prpe.h).
        ``z``: the tap GEMM's output (a tensor), already computed (``x`` is then unused).
        ``out``: as ``conv``'s."""
        taps = self._packs.get(name + ":taps")
        if taps is None:
            taps = pack_upconv_taps(name + ":taps", self.sd[wkey], self.device)
            self._packs[name + ":taps"] = taps
        co = taps.co // 9
        key = name + ":epi"
        if key not in self._aux:
            cb = self.sd[bias_key] if bias_key else None
            if bn is not None:
                s, b = bn_affine(self.sd, bn, BN_EPS, cb)
            else:
                s, b = torch.ones(co), (cb if cb is not None else torch.zeros(co))
            self._aux[key] = s.float().to(self.device)
            self._aux[key + "b"] = b.float().contiguous().to(self.device)
        if z is None:
            z = self.conv(x, taps).t
        B = z.shape[0]
        out = _act(self.empty(B, size[0], size[1], co) if out is None else out)
        slope = self.dev(prelu) if prelu else None
        planes = PLANES_ON and planes and self.precision == 0 and co % 8 == 0 and out.t.is_contiguous()
        # a precision-3/4 consumer reads the output's per-frame max|y| as its activation scale
        ya = self.amax_slot(B) if self.precision in F16_PRECS else None
        args = (z, out.t, align_corners, self._aux[key], self._aux[key + "b"], slope, act)
        self._timed(name + ":upconv", self.up_events, name, (out.t.numel() * 4, z.numel() * 4, planes, act),
                    lambda: ops.upconv3x3(*args, y_planes=planes, y_amax=ya))
        out.amax, out.planes = ya, planes
        return out

    def conv3x3_smallco(self, x, name, wkey, bn=None, bias_key=None, act="none", out=None):
        """3x3 stride-1 pad-1 conv + BN + act for Co <= 4. The direct implicit GEMM re-reads
        the input once per tap for 3 useful output columns; here z = x W_taps (1x1, 9*Co
        outputs, the input read once) and y = act(BN(sum_tap shift_tap(z_tap))) by the tap
        sum of ``upconv`` with the output grid equal to the input grid (align_corners=True at
        unit scale: every source index is exact, interpolation weights 1 and 0). Same
        function as the conv; fp32 summation order differs."""
        if SMALLCO_TAPS:
            return self.upconv(name, x, wkey, x.t.shape[1:3], True, bn=bn, bias_key=bias_key, act=act, out=out)
        return self.conv(x, self.pk(name, wkey, 1, 1, bn=bn, bias_key=bias_key, act=act), out=out)

    # ------------------------------------------------------------------ ResNet-50 trunk
    def trunk(self, x_nchw, flip_w=False):
        """MultiTaskResNetFeatureExtractor (modify_models.py:427-437), torchvision v1.5.
        ``flip_w``: run on the W-mirrored frames (torch.flip(images, dims=[-1]))."""
        with self.prec("trunk"):
            y = self._trunk(x_nchw, flip_w)
            y.epoch = ("trunk", self._amax_epoch.get("trunk"))
            return y

    def feat_prec(self, feat):
        """Precision of a head's first conv over the trunk output ``feat``: 3 (fp32-faithful at
        the 3-term cost) while ``feat``'s per-frame max|x| slots are still the ones its trunk
        call wrote (the trunk pool is re-zeroed by the next trunk call), else the head's own.
        Measured: the face-YOLO adapter's 2048-deep .0 GEMM at precision 0 carried most of the
        box-coordinate error of policy "auto" (tools/yolo_adapter_prec_diag.py)."""
        feat = _act(feat)
        tag = feat.epoch
        if tag is not None and feat.amax is not None and \
                self._amax_epoch.get(tag[0]) == tag[1] and self.policy.get("trunk") == 3:
            return 3
        return None

    def stem(self, x_nchw, flip_w=False, pool=False):
        """conv1 7x7/2 pad 3 + bn1 + relu (torchvision resnet50) as a channel-chunked conv.

        The NCHW frames are copied once into a zero-bordered NHWC4 buffer [B, H+6, W+8, 4]
        (3 rows / columns of padding on each side, 5 extra on the right). Read through the
        overlapping view V[b, h, w, 32] = buf[b, h, w : w+8, 0:4] (pixel stride 4 floats, 32
        "channels" = 8 consecutive columns x 4 channels), the stem is a 7x1-tap, stride-2,
        unpadded conv over 32-channel pixels: one contiguous 128-B row segment per tap, the
        same chunked implicit GEMM as every other conv (and eligible for precision 3). Its
        weight is W'[co][kh*32 + kw*4 + c] = W[co, c, kh, kw] (zero for kw = 7 and c = 3)."""
        B0, _, H0, W0 = x_nchw.shape
        buf = self._batch_buf("stem_buf", B0, (H0 + 6, W0 + 8, 4))
        amax = self.amax_slot(B0) if self.precision == 3 else None
        ops.copy_pad(ops.nhwc(x_nchw), buf[:, 3:3 + H0, 3:3 + W0, :], flip_w=flip_w, y_amax=amax)
        return self._stem_conv(buf, amax, H0, W0, pool)

    def stem_u8(self, frames_u8, ingest, pool=False):
        """``stem`` on uint8 source frames [B, Hs, Ws, 3] (any strides): prpe_frame_ingest resizes,
        pads and normalises them (``ingest``: a prpe.ingest.FrameIngest) straight into the same
        zero-bordered NHWC4 buffer, raising the same per-frame max|x| slots; no fp32 frames exist
        in between. Everything after the fill is ``stem``'s. A sequence of frames [Hs_i, Ws_i, 3]
        of different sizes, or an ``ingest`` with ``antialias=True``, goes through
        prpe_frame_ingest_multi; a 4-D tensor without it takes the one launch of
        prpe_frame_ingest, as before."""
        if isinstance(frames_u8, NV12Frames):
            return self._stem_nv12(frames_u8, ingest, pool)
        multi = not isinstance(frames_u8, torch.Tensor) or ingest.antialias
        frames = ops.frame_list(frames_u8) if multi else frames_u8
        B0 = len(frames)
        H0, W0 = ingest.size
        buf = self._batch_buf("stem_buf", B0, (H0 + 6, W0 + 8, 4))
        amax = self.amax_slot(B0) if self.precision == 3 else None
        if multi:      # frames of different sizes, or the antialias filter: prpe_frame_ingest_multi (§5l)
            ops.frame_ingest_multi(frames, buf[:, 3:3 + H0, 3:3 + W0, :],
                                   [ingest.geometry(*f.shape[:2]) for f in frames], int(ingest.antialias),
                                   ingest.a, ingest.b, ingest.fill, ingest.swap_rb, y_amax=amax)
        else:
            Hs, Ws = frames.shape[1:3]
            ops.frame_ingest(frames, buf[:, 3:3 + H0, 3:3 + W0, :], ingest.geometry(Hs, Ws), ingest.a, ingest.b,
                             ingest.fill, ingest.swap_rb, y_amax=amax)
        return self._stem_conv(buf, amax, H0, W0, pool)

    def _stem_nv12(self, nv12, ingest, pool):
        """``stem_u8`` on a prpe.NV12Frames: prpe_frame_ingest_nv12 converts every
        tap as it gathers it; the output is RGB whatever ``ingest.channel_order`` says of uint8
        sources. With ``ingest.antialias`` the frames are converted first, in the ingest's channel
        order, into a staging buffer this engine owns (one batch size at a time, as the stem
        buffer), and prpe_frame_ingest_multi filters that: the filter's semantics with no new
        filter kernel."""
        B0, Hs, Ws = nv12.shape
        H0, W0 = ingest.size
        buf = self._batch_buf("stem_buf", B0, (H0 + 6, W0 + 8, 4))
        amax = self.amax_slot(B0) if self.precision == 3 else None
        interior = buf[:, 3:3 + H0, 3:3 + W0, :]
        if ingest.antialias:
            key = ("nv12_rgb", B0, Hs, Ws)
            rgb = self._aux.get(key)
            if rgb is None:
                for k in [k for k in self._aux if isinstance(k, tuple) and k[0] == "nv12_rgb"]:
                    del self._aux[k]
                rgb = self._aux[key] = torch.empty(B0, Hs, Ws, 3, device=self.device, dtype=torch.uint8)
            nv12.to_rgb(ingest.channel_order, out=rgb)
            ops.frame_ingest_multi(rgb, interior, [ingest.geometry(Hs, Ws)] * B0, 1, ingest.a, ingest.b, ingest.fill,
                                   ingest.swap_rb, y_amax=amax)
        else:
            ops.frame_ingest_nv12(nv12, interior, ingest.geometry(Hs, Ws), ingest.a, ingest.b, ingest.fill,
                                  y_amax=amax)
        return self._stem_conv(buf, amax, H0, W0, pool)

    def _stem_conv(self, buf, amax, H0, W0, pool):
        """What follows the fill of the stem buffer: the strided view, the pack, the conv (+ pool)."""
        B0 = buf.shape[0]
        # the overlapping view holds the buffer's values and no others: the fill's slots bound it
        v = Act(buf.as_strided((B0, H0 + 6, W0, 32), (buf.stride(0), buf.stride(1), 4, 1)), amax)
        stem = self._packs.get("backbone.conv1")
        if stem is None:
            w = self.sd["backbone.conv1.weight"].float()             # [64, 3, 7, 7]
            wv = torch.zeros(w.shape[0], 7, 8, 4)
            wv[:, :, :7, :3] = w.permute(0, 2, 3, 1)
            s, b = bn_affine(self.sd, "backbone.bn1", BN_EPS)
            stem = pack_matrix("backbone.conv1", wv.reshape(w.shape[0], 7 * 32), 7, 1, 32, 2, 0, self.device,
                               scale=s, bias=b, act="relu", k_order=1)
            self._packs["backbone.conv1"] = stem
        if pool and STEM_POOL and self.precision == 3 and H0 % 4 == 0 and W0 % 4 == 0:
            # + maxpool 3x3/2 pad 1 in the same launch; max-pooling never raises max|x|, so the
            # pooled map's slot is the stem map's maximum (what the unfused path hands on)
            y = self.empty(B0, H0 // 4, W0 // 4, stem.co)
            ya = self.amax_slot(B0)
            name = "backbone.conv1+maxpool"
            self._timed(name, self.events, name, (B0 * (H0 // 2) * (W0 // 2), stem, 3, buf.numel()),
                        lambda: ops.stem_maxpool(buf, H0, W0, amax, stem, y, ya))
            return Act(y, ya, pooled=True)
        return self.conv(v, stem)

    def trunk_u8(self, frames_u8, ingest):
        """``trunk`` on uint8 source frames [B, Hs, Ws, 3] (``stem_u8``): the same kernels from the
        stem conv on, so the same bits as ``trunk`` on fp32 frames holding what the ingest wrote."""
        with self.prec("trunk"):
            y = self._trunk_layers(self.stem_u8(frames_u8, ingest, pool=True))
            y.epoch = ("trunk", self._amax_epoch.get("trunk"))
            return y

    # ---- the per-face crops (prpe.faces): FACE_IMG crops in a stem buffer of their own
    def face_stem_buf(self, n):
        """The stem's zero-bordered NHWC4 buffer for ``n`` face crops, [n, 112+6, 112+8, 4]
        (prpe_roi_resize fills rows / columns 3..114). A kind of its own, as ``crop_pix4``: the
        frames' ``stem_buf`` (batch B) and this one (batch max_crops) alternate without either
        being reallocated."""
        H, W = arch.FACE_IMG
        return self._batch_buf("face_stem_buf", n, (H + 6, W + 8, 4))

    def trunk_from_stem_buf(self, buf, fill, H0, W0):
        """``trunk`` from a stem buffer [n, H0+6, W0+8, 4] that ``fill(interior, amax)`` fills
        inside the trunk's scope: ``interior`` = buf[:, 3:3+H0, 3:3+W0, :], ``amax`` = [n] zeroed
        max|x| slots of the trunk's pool (None below precision 3) that the fill raises, as
        ``stem_u8``'s ingest does. Entering the scope re-zeroes the trunk pool: every head that
        reads an earlier trunk output at ``feat_prec`` must have run before this call."""
        with self.prec("trunk"):
            n = buf.shape[0]
            amax = self.amax_slot(n) if self.precision == 3 else None
            fill(buf[:, 3:3 + H0, 3:3 + W0, :], amax)
            y = self._trunk_layers(self._stem_conv(buf, amax, H0, W0, pool=True))
            y.epoch = ("trunk", self._amax_epoch.get("trunk"))
            return y

    def _trunk(self, x_nchw, flip_w=False):
        return self._trunk_layers(self.stem(x_nchw, flip_w, pool=True))

    def _trunk_layers(self, y):
        if y.pooled:
            x = y
        else:
            B, H, W, C = y.t.shape
            mp = self.empty(B, (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1, C)
            x = Act(ops.maxpool(y.t, mp, 3, 2, 1), y.amax)    # max-pooling never raises max|x|
        for li, (planes, blocks, stride) in enumerate(arch.RESNET50_STAGES, 1):
            for b in range(blocks):
                q = f"backbone.layer{li}.{b}"
                s = stride if b == 0 else 1
                if b > 0 and self._bneck_ok(x, planes):
                    x = self.bottleneck(q, x)
                    continue
                if b == 0 and s == 1 and self._bneck_ok(x, planes, proj=True):
                    x = self.bottleneck(q, x, proj=True)
                    continue
                p1 = self.pk(q + ".conv1", q + ".conv1.weight", bn=q + ".bn1", act="relu")
                if T1_BORDER:
                    # conv1 writes the interior of a zero-bordered buffer and the 3x3 conv2 reads
                    # all of it unpadded (pad 0): same sums (a padded tap adds 0 either way), and
                    # the conv has no tap masks, so it takes conv_wave's pixel-contiguous A loads
                    # (XM 2; csrc/conv_wave.hip)
                    B_, H_, W_, _ = x.t.shape
                    tb = self.bordered(B_, H_, W_, p1.co)
                    o = self.conv(x, p1, out=tb[:, 1:H_ + 1, 1:W_ + 1, :])
                    tb = Act(tb, o.amax)                          # the zero border never raises max|x|
                    o = self.conv(tb, self.pk(q + ".conv2", q + ".conv2.weight", s, 0, bn=q + ".bn2", act="relu"))
                else:
                    o = self.conv(x, p1)
                    o = self.conv(o, self.pk(q + ".conv2", q + ".conv2.weight", s, 1, bn=q + ".bn2", act="relu"))
                if b == 0:
                    # conv3 + bn3 and the downsample projection + its BN summed in one dual-input
                    # GEMM: the projection never goes to HBM as a residual tensor
                    xs = x if s == 1 else Act(x.t[:, ::s, ::s, :], x.amax)    # a subsample never raises max|x|
                    x = self.conv(o, self.pk_dual(q), x2=xs)
                else:
                    x = self.conv(o, self.pk(q + ".conv3", q + ".conv3.weight", bn=q + ".bn3", act="relu"),
                                  res=x, res_mode=RES_PRE)
        return x

    def _bneck_ok(self, x, planes, proj=False):
        return (BNECK_FUSE and (BNECK_PROJ or not proj) and self.precision == 3 and
                (planes == 64 or (planes == 128 and BNECK_L2 and not proj)) and
                x.t.shape[3] == (planes if proj else 4 * planes) and
                x.t.is_contiguous() and x.amax is not None)

    def bottleneck(self, q, x, proj=False):
        """Bottleneck ``q`` (torchvision Bottleneck.forward) as one fused launch (prpe_bottleneck);
        same packs as the unfused path. ``proj``: block 0 of layer1 (stride 1, 64 -> 256 channels),
        whose conv3 + downsample projection run as the dual GEMM of ``pk_dual``."""
        packs = (self.pk(q + ".conv1", q + ".conv1.weight", bn=q + ".bn1", act="relu"),
                 self.pk(q + ".conv2", q + ".conv2.weight", 1, 1, bn=q + ".bn2", act="relu"),
                 self.pk_dual(q) if proj else
                 self.pk(q + ".conv3", q + ".conv3.weight", bn=q + ".bn3", act="relu"))
        B, H, W, _ = x.t.shape
        y = self.empty(B, H, W, packs[2].co)
        ya = self.amax_slot(B)
        self._timed(q, self.events, q, (B * H * W, packs[1], 3, x.t.numel()),
                    lambda: ops.bottleneck(x.t, packs, y, x.amax, ya))
        return Act(y, ya)

    # ------------------------------------------------------------------ YOLO v11n branch
    def yc(self, q, x, k, s=1, act="silu", out=None, res=None, res_mode=0):
        """yolopt Conv: conv -> BN(eps 1e-3) -> act (nn.py:28-36)."""
        p = self.pk(q, q + ".conv.weight", s, k // 2, bn=q + ".norm", eps=YOLO_BN_EPS, act=act)
        return self.conv(x, p, out=out, res=res, res_mode=res_mode)

    def ydw(self, q, x, act="silu", out=None, res=None):
        """depthwise yolopt Conv (g = ch), 3x3 pad 1."""
        key = q + ":dw"
        if key not in self._aux:
            s, b = bn_affine(self.sd, q + ".norm", YOLO_BN_EPS)
            self._aux[key] = self.sd[q + ".conv.weight"].float().reshape(-1).contiguous().to(self.device)
            self._aux[key + "s"] = s.to(self.device)
            self._aux[key + "b"] = b.to(self.device)
        x = _act(x).t
        if out is None:
            out = self.empty(*x.shape)
        return Act(ops.dwconv(x, out, self._aux[key], 3, 1, 1, self._aux[key + "s"], self._aux[key + "b"], act, res))

    def residual(self, q, x, out=None):                       # nn.py:42-49
        t = self.yc(q + ".conv1", x, 3)
        return self.yc(q + ".conv2", t, 3, out=out, res=x, res_mode=RES_POST)

    def cspmodule(self, q, x, out=None):                      # nn.py:52-63
        B, H, W, c = _act(x).t.shape
        Z = self.empty(B, H, W, c)
        h = c // 2
        a = self.yc(q + ".conv1", x, 1)
        self.yc(q + ".conv2", x, 1, out=Z[..., h:])
        a = self.residual(q + ".res_m.0", a)
        self.residual(q + ".res_m.1", a, out=Z[..., :h])
        return self.yc(q + ".conv3", Z, 1, out=out)

    def csp(self, q, x, cout, csp, r, out=None):              # nn.py:66-80 (n = 1)
        B, H, W, _ = _act(x).t.shape
        c = cout // r
        Y = self.empty(B, H, W, 3 * c)
        self.yc(q + ".conv1", x, 1, out=Y[..., :2 * c])
        if csp:
            self.cspmodule(q + ".res_m.0", Y[..., c:2 * c], out=Y[..., 2 * c:])
        else:
            self.residual(q + ".res_m.0", Y[..., c:2 * c], out=Y[..., 2 * c:])
        return self.yc(q + ".conv2", Y, 1, out=out)

    def spp(self, q, x):                                      # nn.py:83-94
        B, H, W, c = _act(x).t.shape
        S = self.empty(B, H, W, 2 * c)
        h = c // 2
        self.yc(q + ".conv1", x, 1, out=S[..., :h])
        for i in range(3):
            ops.maxpool(S[..., i * h:(i + 1) * h], S[..., (i + 1) * h:(i + 2) * h], 5, 1, 2)
        return self.yc(q + ".conv2", S, 1)

    def psa(self, q, x, out=None):                            # nn.py:97-148
        B, H, W, ch = _act(x).t.shape
        T = self.yc(q + ".conv1", x, 1)
        c = ch // 2
        nh = ch // 128
        dh = c // nh
        dk = dh // 2
        y = T.t[..., c:]
        blk = q + ".res_m.0"
        qkv = self.yc(blk + ".conv1.qkv", y, 1, act="none")
        A = self.empty(B, H, W, c)
        V = self.empty(B, H, W, c)
        ops.psa_attention(qkv.t, A, V, nh, dk, dh, dk ** -0.5)
        D = self.ydw(blk + ".conv1.conv1", V, act="none", res=A)            # attn + dwconv(v)
        Y1 = self.yc(blk + ".conv1.conv2", D, 1, act="none", res=y, res_mode=RES_POST)
        Hh = self.yc(blk + ".conv2.0", Y1, 1)
        self.yc(blk + ".conv2.1", Hh, 1, act="none", res=Y1, res_mode=RES_POST, out=T.t[..., c:])
        return self.yc(q + ".conv2", T, 1, out=out)

    def yolo(self, p, feat, stride=(0.0, 0.0, 0.0)):
        """CustomYOLO.forward, eval (modify_models.py:76-106) -> [B, 5, 525]."""
        with self.prec("yolo_adapter"):
            s = self.yolo_adapter(p, feat)
        with self.prec("yolo_net"):
            return self.yolo_net(p, s, stride)

    def yolo_raw(self, p, x_nchw, stride=(0.0, 0.0, 0.0)):
        """yolopt ``YOLO.forward`` eval (nn.py:294-297) straight on frames [B,3,H,W] (NCHW,
        read in place through an NHWC view): the config-2 micro-bench variant, A = 8400 at
        640x640 -> [B, 5, A]."""
        with self.prec("yolo_net"):
            return self.yolo_net(p, ops.nhwc(x_nchw), stride)

    def yolo_adapter(self, p, feat):
        a = p + ".adapter"
        t = self.conv(feat, self.pk(a + ".0", a + ".0.weight", bn=a + ".1", bias_key=a + ".0.bias", act="silu"),
                      prec=self.feat_prec(feat))
        p7 = self.pk(a + ".7", a + ".7.weight", bn=a + ".8", bias_key=a + ".7.bias", act="silu")
        u = self.upconv(a + ".4", t, a + ".4.weight", arch.YOLO_IMG, True, bn=a + ".5", bias_key=a + ".4.bias",
                        act="silu", planes=True)
        t = self.conv(u, p7, planes_out=True)
        p10 = self.pk(a + ".10", a + ".10.weight", 1, 1, bn=a + ".11", bias_key=a + ".10.bias", act="silu")
        if SMALLCO_TAPS and TAPS_FUSE and t.planes:
            # .10's epilogue runs .13 (1x1 128->64 + BN + SiLU) and .16's tap GEMM (64 -> 27):
            # neither the 128- nor the 64-channel map reaches HBM (prpe.h, w2 / w3)
            w2 = self.dev(a + ".13:w", lambda: self.sd[a + ".13.weight"].float().flatten(1))
            s2 = self.dev(a + ".13:s", lambda: bn_affine(self.sd, a + ".14", BN_EPS, self.sd[a + ".13.bias"])[0])
            b2 = self.dev(a + ".13:b", lambda: bn_affine(self.sd, a + ".14", BN_EPS, self.sd[a + ".13.bias"])[1])
            w3 = self.dev(a + ".16:w2", lambda: self.sd[a + ".16.weight"].float().permute(2, 3, 0, 1)
                          .reshape(-1, w2.shape[0]).contiguous())
            B, H, W, _ = t.t.shape
            z = self.empty(B, H, W, w3.shape[0])
            sink = self.dev("sink:" + str(p10.co), lambda: torch.zeros(p10.co)).expand(B, H, W, p10.co)
            self.conv(t, p10, out=sink, w2=w2, y2=z, w3=w3, scale2=s2, bias2=b2, act2="silu")
            t = self.upconv(a + ".16", None, a + ".16.weight", (H, W), True, bn=a + ".17", bias_key=a + ".16.bias",
                            act="silu", z=z)
            return Act(ops.norm_sigmoid(t.t, self.empty(*t.t.shape)))
        # .10 and .13 write fp32: the 64-column 1x1 below runs faster on the register-staged
        # 256x64 tile than on the planes-input wave tile (1.12 vs 1.64 ms at bs=256), and the
        # 27-column tap GEMM after .13 needs fp32 input
        t = self.conv(t, p10)
        t = self.conv(t, self.pk(a + ".13", a + ".13.weight", bn=a + ".14", bias_key=a + ".13.bias", act="silu"))
        t = self.conv3x3_smallco(t, a + ".16", a + ".16.weight", bn=a + ".17", bias_key=a + ".16.bias",
                                 act="silu")
        return Act(ops.norm_sigmoid(t.t, self.empty(*t.t.shape)))

    def yolo_net(self, p, s, stride):
        B = _act(s).t.shape[0]
        n = p + ".yolo.net"
        x = self.yc(n + ".p1.0", s, 3, 2)
        x = self.csp(n + ".p2.1", self.yc(n + ".p2.0", x, 3, 2), 64, False, 4)
        x = self.yc(n + ".p3.0", x, 3, 2)
        _, H3, W3, _ = x.t.shape
        F2 = self.empty(B, H3, W3, 256)                     # cat(up(h1), p3)
        p3 = self.csp(n + ".p3.1", x, 128, False, 4, out=F2[..., 128:])
        x = self.yc(n + ".p4.0", p3, 3, 2)
        _, H4, W4, _ = x.t.shape
        F1 = self.empty(B, H4, W4, 384)                     # cat(up(p5), p4)
        p4 = self.csp(n + ".p4.1", x, 128, True, 2, out=F1[..., 256:])
        x = self.csp(n + ".p5.1", self.yc(n + ".p5.0", p4, 3, 2), 256, True, 2)
        x = self.spp(n + ".p5.2", x)
        _, H5, W5, _ = x.t.shape
        F4 = self.empty(B, H5, W5, 384)                     # cat(h5(p4''), p5)
        p5 = self.psa(n + ".p5.3", x, out=F4[..., 128:])
        f = p + ".yolo.fpn"
        ops.upsample_nearest2x(p5.t, F1[..., :256])
        F3 = self.empty(B, H4, W4, 192)                     # cat(h3(p3'), p4')
        h1 = self.csp(f + ".h1", F1, 128, False, 2, out=F3[..., 64:])
        ops.upsample_nearest2x(h1.t, F2[..., :128])
        P3 = self.csp(f + ".h2", F2, 64, False, 2)
        self.yc(f + ".h3", P3, 3, 2, out=F3[..., :64])
        P4 = self.csp(f + ".h4", F3, 128, False, 2)
        self.yc(f + ".h5", P4, 3, 2, out=F4[..., :128])
        P5 = self.csp(f + ".h6", F4, 256, True, 2)
        return self.head(p + ".yolo.head", (P3, P4, P5), stride)

    def head(self, h, feats, stride):
        """Head eval (nn.py:255-270): box/cls convs per level -> one [B, A, 65] buffer -> DFL decode."""
        B = feats[0].t.shape[0]
        A = sum(x.t.shape[1] * x.t.shape[2] for x in feats)
        HEAD = self.empty(B, A, 65)
        off = 0
        hw = []
        for i, x in enumerate(feats):
            _, H, W, _ = x.t.shape
            hv = HEAD[:, off:off + H * W, :].view(B, H, W, 65)
            t = self.yc(f"{h}.box.{i}.1", self.yc(f"{h}.box.{i}.0", x, 3), 3)
            self.conv(t, self.pk(f"{h}.box.{i}.2", f"{h}.box.{i}.2.weight", bias_key=f"{h}.box.{i}.2.bias"),
                      out=hv[..., :64])
            t = self.ydw(f"{h}.cls.{i}.0", x)
            t = self.yc(f"{h}.cls.{i}.1", t, 1)
            t = self.ydw(f"{h}.cls.{i}.2", t)
            t = self.yc(f"{h}.cls.{i}.3", t, 1)
            self.conv(t, self.pk(f"{h}.cls.{i}.4", f"{h}.cls.{i}.4.weight", bias_key=f"{h}.cls.{i}.4.bias"),
                      out=hv[..., 64:])
            hw.append((H, W))
            off += H * W
        det = self.empty(B, 5, A)
        return ops.dfl_decode(HEAD, det, 1, hw, [float(s) for s in stride])

    # ------------------------------------------------------------------ AdaFace / IR-50
    def adaface(self, feat):
        """CustomAdaFace.forward (modify_models.py:288-297) -> (emb [B,512], norm [B,1])."""
        with self.prec("adaface"):
            return self._adaface(feat)

    def _adaface(self, feat):
        a = "ada_face.adapter"
        t = self.conv(feat, self.pk(a + ".0", a + ".0.weight", bn=a + ".1", bias_key=a + ".0.bias", act="prelu",
                                    prelu=a + ".2.weight"), prec=self.feat_prec(feat))
        u = self.upconv(a + ".4", t, a + ".4.weight", (112, 112), True, bn=a + ".5", bias_key=a + ".4.bias",
                        act="prelu", prelu=a + ".6.weight", planes=True)
        t = self.conv(u, self.pk(a + ".7", a + ".7.weight", 1, 1, bn=a + ".8", bias_key=a + ".7.bias", act="prelu",
                                 prelu=a + ".9.weight"), planes_out=True)
        t = self.conv(t, self.pk(a + ".10", a + ".10.weight", 1, 1, bn=a + ".11", bias_key=a + ".10.bias",
                                 act="prelu", prelu=a + ".12.weight"), planes_out=True)
        m = "ada_face.adaface_model"
        x = self.conv(t, self.pk(m + ".input_layer", m + ".input_layer.0.weight", 1, 1, bn=m + ".input_layer.1",
                                 act="prelu", prelu=m + ".input_layer.2.weight"))
        for i, (cin, d, st) in enumerate(arch.IR50_UNITS):
            q = f"{m}.body.{i}"
            if cin == d:
                sc = x.t[:, ::st, ::st, :]                    # MaxPool2d(1, st) == subsample
            else:
                sc = self.conv(x, self.pk(q + ".shortcut", q + ".shortcut_layer.0.weight", st, 0,
                                          bn=q + ".shortcut_layer.1"))
            r = self.conv(x, self.pk(q + ".res1", q + ".res_layer.1.weight", 1, 1, bn=q + ".res_layer.2",
                                     act="prelu", prelu=q + ".res_layer.3.weight", in_bn=q + ".res_layer.0"))
            x = self.conv(r, self.pk(q + ".res4", q + ".res_layer.4.weight", st, 1, bn=q + ".res_layer.5"),
                          res=sc, res_mode=RES_PRE)
        # output_layer: BN2d (prologue) -> Dropout(eval: id) -> Flatten(NCHW) -> Linear -> BN1d
        lin = self._packs.get("ir50.output")
        if lin is None:
            sd = self.sd
            w = sd[m + ".output_layer.3.weight"].float().view(512, 512, 7, 7)   # NCHW flatten order
            s1, b1 = bn_affine(sd, m + ".output_layer.4", BN_EPS, sd[m + ".output_layer.3.bias"])
            in_s, in_b = bn_affine(sd, m + ".output_layer.0", BN_EPS)
            # M = frames (one output pixel each), K = 25,088: tap-major weights (k = the NHWC
            # flatten order) for the automatic split-K path (conv_splitk.hip: one K-slice per tap,
            # 392 workgroups at bs = 256); PRPE_IR50_OUT_TILE=4 runs the round-1 choice instead
            # (the 128x16 register-staged tile, 64 blocks, chunk-major weights)
            tile = int(os.environ.get("PRPE_IR50_OUT_TILE", "0"))
            lin = pack_conv("ir50.output", w, 1, 0, self.device, scale=s1, bias=b1, in_scale=in_s, in_bias=in_b,
                            k_order=0 if tile == 0 else "auto")
            lin.tile = tile
            self._packs["ir50.output"] = lin
        B = x.t.shape[0]
        y = self.conv(x, lin, prec=0, track=False).t         # [B,1,1,512]
        emb = self.empty(B, 512)
        norm = self.empty(B, 1)
        ops.l2norm(y.view(B, 512), emb, norm)
        return emb, norm

    # ------------------------------------------------------------------ ViTPose-B
    def vit_adapter(self, feat):
        """CustomVitPose.adapter (modify_models.py:352-374) -> pixel_values NHWC [B,256,192,3]."""
        a = "vit_pose.adapter"
        t = self.conv(feat, self.pk(a + ".0", a + ".0.weight", bn=a + ".1", bias_key=a + ".0.bias", act="gelu"),
                      prec=self.feat_prec(feat))
        u = self.upconv(a + ".4", t, a + ".4.weight", arch.VIT_IMG, True, bn=a + ".5", bias_key=a + ".4.bias",
                        act="gelu", planes=True)
        p7 = self.pk(a + ".7", a + ".7.weight", 1, 1, bn=a + ".8", bias_key=a + ".7.bias", act="gelu")
        if SMALLCO_TAPS and TAPS_FUSE and u.planes:
            # .7's epilogue computes .10's tap GEMM (w2 = .10's weight as [(tap, co), ci], the
            # pack_upconv_taps order); its 128-channel output exists only in LDS
            w2 = self.dev(a + ".10:w2", lambda: self.sd[a + ".10.weight"].float().permute(2, 3, 0, 1)
                          .reshape(-1, p7.co).contiguous())
            B, H, W, _ = u.t.shape
            z = self.empty(B, H, W, w2.shape[0])
            sink = self.dev("sink:" + str(p7.co), lambda: torch.zeros(p7.co)).expand(B, H, W, p7.co)
            self.conv(u, p7, out=sink, w2=w2, y2=z)
            out = self._vit_pix_out(B)
            return self.upconv(a + ".10", None, a + ".10.weight", (H, W), True, bn=a + ".11",
                               bias_key=a + ".10.bias", act="gelu", z=z, out=out)
        t = self.conv(u, p7)
        return self.conv3x3_smallco(t, a + ".10", a + ".10.weight", bn=a + ".11", bias_key=a + ".10.bias",
                                    act="gelu", out=self._vit_pix_out(t.t.shape[0]))

    # ---- the ViTPose crops in a zero-bordered NHWC4 buffer [B, 256+4, 192+4, 4] (2 rows / columns
    # of padding = the patch conv's pad, the 4th channel 0): the adapter's last conv writes the
    # interior, the patch embedding reads the overlapping view of vit_pix4 (as the stem's buffer)
    def vit_pix4(self, B):
        H, W = arch.VIT_IMG
        return self._batch_buf("vit_pix4", B, (H + 4, W + 4, 4))

    def _vit_pix_out(self, B):
        return self.pix4_interior(self.vit_pix4(B)) if PATCH_VIEW else None

    def crop_pix4(self, n):
        """The top-down crops (prpe.topdown): the zero-bordered NHWC4 buffer [n, 260, 196, 4]
        prpe_crop_resize fills. A kind of its own: _batch_buf keeps one batch size per kind, so
        sharing vit_pix4's would reallocate whenever whole-frame pose (batch B) and top-down pose
        (batch max_crops) alternate."""
        H, W = arch.VIT_IMG
        return self._batch_buf("crop_pix4", n, (H + 4, W + 4, 4))

    @staticmethod
    def pix4_interior(buf):
        """The pixel_values view [n, 256, 192, 3] of a pix4 buffer (or of its first n slots) as an
        Act that names the buffer, so that vit_backbone reads it in place instead of copying into
        vit_pix4."""
        H, W = arch.VIT_IMG
        return Act(buf[:, 2:2 + H, 2:2 + W, :3], pix4=buf)

    def _lin(self, name, wkey, bkey, act="none"):
        p = self._packs.get(name)
        if p is None:
            w = self.sd[wkey] if isinstance(wkey, str) else torch.cat([self.sd[k] for k in wkey], 0)
            b = self.sd[bkey] if isinstance(bkey, str) else torch.cat([self.sd[k] for k in bkey], 0)
            p = pack_matrix(name, w, 1, 1, w.shape[1], 1, 0, self.device, bias=b, act=act)
            self._packs[name] = p
        return p

    def vit_backbone(self, pix):
        """VitPoseForPoseEstimation.forward (modeling_vitpose.py:190-278) -> heatmaps [B,17,64,48]."""
        v = "vit_pose.vit_pose.backbone"
        pix = _act(pix)
        B = pix.t.shape[0]
        Hp, Wp = arch.VIT_GRID
        L, D = Hp * Wp, arch.VIT_HIDDEN
        pos = self.dev("vit.possum", lambda: (self.sd[v + ".embeddings.position_embeddings"][0, 1:] +
                                              self.sd[v + ".embeddings.position_embeddings"][0, :1]))
        X = self.empty(B, Hp, Wp, D)
        pos_v = pos.view(1, Hp, Wp, D).expand(B, Hp, Wp, D)
        if PATCH_VIEW:
            # the 16x16/16 pad-2 patch conv over 3 channels as a 16x1/16 conv over 64-"channel" pixels:
            # V[b, h, w, 0:64] = P4[b, h, w : w+16, 0:4] (pixel stride 4 floats), P4 the zero-bordered
            # NHWC4 crops (the padding is the conv's); W'[co][kw*4 + c][kh] = W[co, c, kh, kw] (0 for
            # c = 3). One contiguous 256-B row segment per tap row: the chunked implicit GEMM
            P4 = pix.pix4
            if P4 is None:                             # pixel_values from the caller (config 3)
                P4 = self.vit_pix4(B)
                ops.copy_pad(pix.t, P4[:, 2:2 + pix.t.shape[1], 2:2 + pix.t.shape[2], :])
            Hv, Wv = P4.shape[1], (Wp - 1) * arch.VIT_PATCH + 1
            V = P4.as_strided((B, Hv, Wv, 64), (P4.stride(0), P4.stride(1), 4, 1))
            patch = self._packs.get("vit.patch4")
            if patch is None:
                w = self.sd[v + ".embeddings.patch_embeddings.projection.weight"].float()    # [768, 3, 16, 16]
                wv = torch.zeros(w.shape[0], 16, 16, 4)
                wv[..., :3] = w.permute(0, 2, 3, 1)                                        # [co, kh, kw, c]
                w4 = wv.permute(0, 2, 3, 1).reshape(w.shape[0], 64, 16, 1)                # [co, kw*4 + c, kh, 1]
                patch = pack_conv("vit.patch4", w4, 16, 0, self.device,
                                  bias=self.sd[v + ".embeddings.patch_embeddings.projection.bias"])
                self._packs["vit.patch4"] = patch
            self.conv(V, patch, out=X, res=pos_v, res_mode=RES_PRE)
        else:
            patch = self.pk("vit.patch", v + ".embeddings.patch_embeddings.projection.weight", 16, 2,
                            bias_key=v + ".embeddings.patch_embeddings.projection.bias")
            self.conv(pix, patch, out=X, res=pos_v, res_mode=RES_PRE)
        X2 = X.view(B * L, D)
        as4 = lambda t: t.view(t.shape[0], 1, 1, t.shape[1])

        # the producer wrote the planes format, which a reshape keeps: the GEMM consumer reads it without a split
        as4p = lambda t: Act(as4(t), planes=pl)
        # LayerNorm and attention write their outputs in the planes format when precision 0
        # consumes them (qkv / fc1 / proj GEMMs: the operand split done once by the producer)
        pl = PLANES_ON and self.precision == 0
        Hh, Dh = arch.VIT_HEADS, D // arch.VIT_HEADS
        for i in range(arch.VIT_LAYERS):
            q = f"{v}.encoder.layer.{i}"
            A = q + ".attention.attention"
            hn = ops.layernorm(X2, self.empty(B * L, D), self.dev(q + ".layernorm_before.weight"),
                               self.dev(q + ".layernorm_before.bias"), planes=pl)
            qkv = self.conv(as4p(hn), self._lin(q + ":qkv", [A + ".query.weight", A + ".key.weight", A + ".value.weight"],
                                                [A + ".query.bias", A + ".key.bias", A + ".value.bias"]))
            ctx = ops.attention_strided(qkv.t, (L * 3 * D, D, Dh, 3 * D), self.empty(B * L, D), B, L, Hh, Dh,
                                        Dh ** -0.5, out_planes=pl)
            X2 = self.conv(as4p(ctx), self._lin(q + ":proj", q + ".attention.output.dense.weight",
                                                q + ".attention.output.dense.bias"),
                           res=as4(X2), res_mode=RES_PRE).t.view(B * L, D)
            hn = ops.layernorm(X2, self.empty(B * L, D), self.dev(q + ".layernorm_after.weight"),
                               self.dev(q + ".layernorm_after.bias"), planes=pl)
            f1 = self.conv(as4p(hn), self._lin(q + ":fc1", q + ".mlp.fc1.weight", q + ".mlp.fc1.bias", act="gelu"),
                           planes_out=True)
            X2 = self.conv(f1, self._lin(q + ":fc2", q + ".mlp.fc2.weight", q + ".mlp.fc2.bias"),
                           res=as4(X2), res_mode=RES_PRE).t.view(B * L, D)
        hn = ops.layernorm(X2, self.empty(B * L, D), self.dev(v + ".layernorm.weight"), self.dev(v + ".layernorm.bias"),
                           relu=True)
        heat = self.empty(B, arch.NUM_KEYPOINTS, *arch.HEATMAP)
        self.upconv("vit.head", hn.view(B, Hp, Wp, D), "vit_pose.vit_pose.head.conv.weight", arch.HEATMAP, False,
                    bias_key="vit_pose.vit_pose.head.conv.bias", out=ops.nhwc(heat))
        return heat

    def vitpose(self, feat):
        with self.prec("vit"):
            return self.vit_backbone(self.vit_adapter(feat))

    # ------------------------------------------------------------------ warm-up
    def prepare(self, tasks=arch.TASKS):
        """Build every weight pack once (so timed regions contain kernels only)."""
        x = torch.zeros(1, 3, 64, 64, device=self.device)
        # the heads run on this trunk output (its max|x| slots tagged), so every conv takes the
        # precision it takes in a real forward -- the adapters' .0 GEMMs precision 3 (feat_prec) --
        # and every fp16 weight plane is built here, not lazily inside a timed forward (the
        # adapters upsample to fixed sizes, so a 2x2 feature map exercises the same packs)
        feat = self.trunk(x)
        if "face_detection" in tasks:
            self.yolo("yolo_face", feat)
        if "person_detection" in tasks:
            self.yolo("yolo_person", feat)
        if "face_recognition" in tasks:
            self.adaface(feat)
        if "pose_estimation" in tasks:
            self.vitpose(feat)
        del feat
        torch.cuda.synchronize(self.device)
