"""GPU: every stage of prpe.engine.Engine against the fp64 oracle, tap by tap, at the smallest frame
sizes that reach each route (the cases and the oracle: tests/test_stage_parity_host.py).

The end-to-end tests compare final outputs at 640x640 with 1e-3 bars. A trunk conv that loses a
split term, or reads another frame's max|x| slot, moves the result by far less than that. Here the
engine's stage entry points (trunk, trunk_u8, trunk_from_stem_buf, yolo_adapter, yolo_net, adaface,
vit_adapter, vit_backbone) are driven directly, from the same fp32 input as the oracle, and

    err(tap) = max|gpu - fp64| / max|fp64|

is judged against e_ref(tap), the fp32 CPU oracle's own error at that tap.

Taps are taken without changing what is launched: Engine.conv / bottleneck / upconv / head and a
few prpe.ops functions are wrapped (monkeypatch) and the returned tensor is cloned under its pack
name. A planes-format output (bf16 hi / lo, include/prpe.h) is decoded as hi + lo. A tap that a
fused launch keeps in LDS does not exist on the device; those are named per route
(check_trunk_routes, head_fused_away: the stem map under the fused stem + pool, the ViTPose
adapter's .7 under its fused tap GEMM), and every other tap of the host list must be there.

Sizes (trunk batch 3, heads batch 2):
  64x96        the pipelines' size: fused stem + pool, fused bottlenecks, a 2x3 feature
  112x112      trunk_from_stem_buf (the face-crop trunk), filled by a plain copy, a 4x4 feature
  70x54        H % 4 != 0 and W % 4 != 0: stem conv and max-pool apart, odd dimensions at every
               stride-2 stage, a non-trivial ``::s`` subsample view
  96x136_flip  flip_w=True against the oracle on the flipped frames
  64x96_u8     trunk_u8 with an identity-geometry ingest against the oracle on v * a + b

Per tap: (1) err, e_ref and err / e_ref are printed; (2) where the Act has max|x| slots,
amax[n] >= max|t[n]| exactly, for every frame; (3) the bound below; (4) two runs give the same bits.
Per run: the launches recorded from prpe.ops show the routes the policy is there for.

Bounds. Precision 2 and 3 stages: err <= c * e_ref with c = twice the measured maximum of
err / e_ref at that tap rounded up to a power of two (RATIO; DESIGN.md §3, "Stage parity"),
never above 16: one bf16-split step down is 2^-17 per operand against fp32's 2^-24, a factor of
128, so beyond 16 x e_ref is a lost term or a wrong scale, not summation order. Precision 0 and 4
stages (the "auto" heads): err <= twice the err measured on the MI355X (ERR_AUTO, same table), and
the final taps keep the 1e-3 end-to-end bars as a ceiling.
"""
import pytest
import torch

import test_stage_parity_host as H
from prpe import engine as E
from prpe import ops
from prpe.ingest import FrameIngest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 16.0

# The largest err / e_ref measured on the MI355X at each tap of a precision 2 or 3 stage, over the
# sizes and policies that run it so (DESIGN.md §3 "Stage parity" gives the per-stage maxima of
# these). Asserted: err <= c * e_ref with c = 2 x this, rounded up to a power of two, at most CAP.
RATIO = {
    'backbone.maxpool': 1.24,
    'backbone.layer1.0': 1.09,
    'backbone.layer1.1': 1.17,
    'backbone.layer1.2': 1.11,
    'backbone.layer2.0': 1.32,
    'backbone.layer2.1': 1.35,
    'backbone.layer2.2': 1.43,
    'backbone.layer2.3': 1.31,
    'backbone.layer3.0': 1.69,
    'backbone.layer3.1': 1.66,
    'backbone.layer3.2': 1.73,
    'backbone.layer3.3': 1.94,
    'backbone.layer3.4': 1.83,
    'backbone.layer3.5': 1.82,
    'backbone.layer4.0': 2.6,
    'backbone.layer4.1': 2.55,
    'backbone.layer4.2': 2.7,
    'backbone.conv1': 1.24,
    'yolo_face.adapter': 1.63,
    'yolo_face.yolo.fpn.P3': 0.957,
    'yolo_face.yolo.fpn.P4': 0.691,
    'yolo_face.yolo.fpn.P5': 0.652,
    'yolo_face.yolo.head.raw': 0.658,
    'yolo_face.det.box': 1.08,
    'yolo_face.det.cls': 1.29,
    'ada_face.adapter.0': 5.47,
    'ada_face.adapter.4': 1.86,
    'ada_face.adapter.7': 3.35,
    'ada_face.adapter.10': 2.64,
    'ada_face.adaface_model.input_layer': 2.25,
    'ada_face.adaface_model.body.2': 2.26,
    'ada_face.adaface_model.body.6': 2.14,
    'ada_face.adaface_model.body.20': 3.27,
    'ada_face.adaface_model.body.23': 2.14,
    'ada_face.adaface_model.output': 2.79,
    'ada_face.norm': 3.04,
    'ada_face.emb': 2.8,
    'vit_pose.adapter.0': 3.3,
    'vit_pose.adapter.4': 1.71,
    'vit_pose.adapter.7': 3.14,
    'vit_pose.adapter.10': 2.35,
    'vit_pose.vit_pose.backbone.embeddings': 1.02,
    'vit_pose.vit_pose.backbone.encoder.layer.0': 1.12,
    'vit_pose.vit_pose.backbone.encoder.layer.5': 2.35,
    'vit_pose.vit_pose.backbone.encoder.layer.11': 2.28,
    'vit_pose.vit_pose.backbone.layernorm': 2.25,
    'vit_pose.heatmaps': 2.53,
}
# err measured on the MI355X at policy "auto" for the taps of precision 0 / 4 stages (the larger of
# the two sizes; DESIGN.md §3 "Stage parity", column err at "auto"); asserted at twice this
ERR_AUTO = {
    'yolo_face.adapter': 0.000152,
    'ada_face.adapter.0': 1.03e-06,
    'ada_face.adapter.4': 0.000415,
    'ada_face.adapter.7': 0.000524,
    'ada_face.adapter.10': 0.000967,
    'ada_face.adaface_model.input_layer': 0.000689,
    'ada_face.adaface_model.body.2': 0.000823,
    'ada_face.adaface_model.body.6': 0.00123,
    'ada_face.adaface_model.body.20': 0.0013,
    'ada_face.adaface_model.body.23': 0.00128,
    'ada_face.adaface_model.output': 0.00147,
    'ada_face.norm': 0.00018,
    'ada_face.emb': 0.00131,
    'vit_pose.adapter.0': 1.02e-06,
    'vit_pose.adapter.4': 8.28e-06,
    'vit_pose.adapter.10': 2.8e-05,
    'vit_pose.vit_pose.backbone.embeddings': 3.81e-06,
    'vit_pose.vit_pose.backbone.encoder.layer.0': 5.16e-06,
    'vit_pose.vit_pose.backbone.encoder.layer.5': 8.33e-06,
    'vit_pose.vit_pose.backbone.encoder.layer.11': 1.03e-05,
    'vit_pose.vit_pose.backbone.layernorm': 1.32e-05,
    'vit_pose.heatmaps': 1.16e-05,
}
# the same for the heads' first stages on a stale trunk feature (their .0 conv at the head's own
# precision instead of feat_prec's 3)
ERR_STALE = {
    'yolo_face.adapter': 0.000134,
    'ada_face.adapter.0': 5.74e-06,
    'ada_face.adapter.4': 0.000426,
    'ada_face.adapter.7': 0.000522,
    'ada_face.adapter.10': 0.000944,
    'ada_face.adaface_model.input_layer': 0.000677,
    'ada_face.adaface_model.body.2': 0.000677,
    'ada_face.adaface_model.body.6': 0.001,
    'ada_face.adaface_model.body.20': 0.00104,
    'ada_face.adaface_model.body.23': 0.000959,
    'ada_face.adaface_model.output': 0.00114,
    'ada_face.norm': 0.000104,
    'ada_face.emb': 0.000808,
    'vit_pose.adapter.0': 7.07e-06,
    'vit_pose.adapter.4': 9.78e-06,
    'vit_pose.adapter.10': 4.29e-05,
}
# the 1e-3 absolute end-to-end bars, a ceiling on the final taps whatever was measured
FINAL_ABS = {"vit_pose.heatmaps": 1e-3, "ada_face.emb": 1e-3, H.YOLO + ".det.cls": 1e-3}
FINAL_REL = {H.YOLO + ".det.box": 2e-3, "ada_face.norm": 1e-3}        # x max|box|; norms relative

# stage -> the policy component its convs run under
COMP = {"yolo_adapter": "yolo_adapter", "yolo_net": "yolo_net", "adaface": "adaface", "vit_adapter": "vit",
        "vit_backbone": "vit"}
# pack name (Engine.conv / upconv) -> (tap, layout); "rows": the tensor reshapes to the oracle's
_A, _M, _V, _VA = H._A, H._M, H._V, H._VA
CONV_TAPS = {"backbone.conv1": ("backbone.conv1", "nhwc"), "ir50.output": (_M + ".output", "rows"),
             "vit.patch4": (_V + ".embeddings", "rows"), _M + ".input_layer": (_M + ".input_layer", "nhwc")}
for _q in H.TRUNK_BLOCKS:
    CONV_TAPS[_q + ".conv3"] = CONV_TAPS[_q + ".conv3+downsample"] = (_q, "nhwc")
for _q in (_A + ".0", _A + ".7", _A + ".10", _VA + ".0", _VA + ".7"):
    CONV_TAPS[_q] = (_q, "nhwc")
for _i in (2, 6, 20, 23):
    CONV_TAPS[f"{_M}.body.{_i}.res4"] = (f"{_M}.body.{_i}", "nhwc")
for _i in (0, 5, 11):
    CONV_TAPS[f"{_V}.encoder.layer.{_i}:fc2"] = (f"{_V}.encoder.layer.{_i}", "rows")
UPCONV_TAPS = {_A + ".4": _A + ".4", _VA + ".4": _VA + ".4", _VA + ".10": _VA + ".10"}


class Tap:
    def __init__(self, t, layout, amax=None, planes=False):
        self.t = t.detach().clone()                      # the logical tensor, dense
        self.layout, self.planes = layout, planes
        self.amax = None if amax is None else amax.detach().clone()

    def value(self, shape):
        """fp32 CPU tensor in the oracle's layout and shape."""
        t = self.t.cpu()
        if self.planes:                                  # hi + lo of the two-plane bf16 split
            n, h, w, c = t.shape
            u = t.contiguous().view(torch.int16).view(n, h, w, c // 8, 2, 8)
            hi, lo = (u[..., i, :].contiguous().view(torch.bfloat16).float().reshape(n, h, w, c) for i in (0, 1))
            t = hi + lo
        if self.layout == "nhwc":
            t = t.permute(0, 3, 1, 2)
        return t.reshape(shape)


class Recorder:
    """Wraps the engine's layer methods and the ops the stages call: ``taps`` (name -> Tap) and
    ``launches`` (one tuple per recorded library call)."""

    def __init__(self, monkeypatch):
        self.taps, self.launches = {}, []
        rec = self
        conv0, bneck0, up0, head0 = E.Engine.conv, E.Engine.bottleneck, E.Engine.upconv, E.Engine.head

        def conv(eng, x, p, *a, **kw):
            out = conv0(eng, x, p, *a, **kw)
            if p.name in CONV_TAPS and kw.get("w2") is None:
                name, layout = CONV_TAPS[p.name]
                rec.taps[name] = Tap(out.t, layout, out.amax, out.planes)
            return out

        def bottleneck(eng, q, x, *a, **kw):
            out = bneck0(eng, q, x, *a, **kw)
            rec.taps[q] = Tap(out.t, "nhwc", out.amax)
            return out

        def upconv(eng, name, *a, **kw):
            out = up0(eng, name, *a, **kw)
            if name in UPCONV_TAPS:
                rec.taps[UPCONV_TAPS[name]] = Tap(out.t, "nhwc", out.amax, out.planes)
            return out

        def head(eng, h, feats, stride):
            for i, f in enumerate(feats):
                rec.taps[f"{H.YOLO}.yolo.fpn.P{i + 3}"] = Tap(f.t, "nhwc", f.amax, f.planes)
            return head0(eng, h, feats, stride)

        for k, f in (("conv", conv), ("bottleneck", bottleneck), ("upconv", upconv), ("head", head)):
            monkeypatch.setattr(E.Engine, k, f)

        conv2d0, bn0, sm0, mp0, ln0, dfl0 = (ops.conv2d, ops.bottleneck, ops.stem_maxpool, ops.maxpool,
                                             ops.layernorm, ops.dfl_decode)

        def conv2d(x, pack, y, **kw):
            xa, x2 = kw.get("x_amax"), kw.get("x2")
            rec.launches.append(("conv2d", pack.name, kw.get("precision", 0), pack.pad, None if xa is None else
                                 xa.data_ptr(), None if x2 is None else x2.is_contiguous(), tuple(x.shape)))
            return conv2d0(x, pack, y, **kw)

        def bottleneck_op(x, packs, y, x_amax, y_amax=None):
            rec.launches.append(("bottleneck", packs[0].name))
            return bn0(x, packs, y, x_amax, y_amax)

        def stem_maxpool(buf, h, w, x_amax, pack, y, y_amax=None):
            out = sm0(buf, h, w, x_amax, pack, y, y_amax)
            rec.launches.append(("stem_maxpool",))
            rec.taps["backbone.maxpool"] = Tap(y, "nhwc", y_amax)
            return out

        def maxpool(x, y, k, stride, pad):
            out = mp0(x, y, k, stride, pad)
            if (k, stride, pad) == (3, 2, 1):
                rec.launches.append(("maxpool",))
                rec.taps["backbone.maxpool"] = Tap(y, "nhwc")
            return out

        def layernorm(x2d, y2d, gamma, beta, eps=1e-12, relu=False, planes=False):
            out = ln0(x2d, y2d, gamma, beta, eps, relu, planes)
            if relu:                                     # the final LayerNorm (+ the decoder's ReLU)
                rec.taps[_V + ".layernorm"] = Tap(y2d, "rows", planes=planes)
            return out

        def dfl_decode(head, out, nc, level_hw, strides):
            rec.taps[H.YOLO + ".yolo.head.raw"] = Tap(head.transpose(1, 2), "rows")
            return dfl0(head, out, nc, level_hw, strides)

        for k, f in (("conv2d", conv2d), ("bottleneck", bottleneck_op), ("stem_maxpool", stem_maxpool),
                     ("maxpool", maxpool), ("layernorm", layernorm), ("dfl_decode", dfl_decode)):
            monkeypatch.setattr(ops, k, f)

    def reset(self):
        self.taps, self.launches = {}, []

    def convs(self, prefix=""):
        return [l for l in self.launches if l[0] == "conv2d" and l[1].startswith(prefix)]


@pytest.fixture(scope="module")
def engine_of(state_dict):
    engines = {}

    def get(policy):
        if policy not in engines:
            engines[policy] = E.Engine(state_dict, device=DEV, precision=policy)
        return engines[policy]
    return get


@pytest.fixture(autouse=True)
def _default_switches():
    off = [s for s in ("PLANES_ON", "SMALLCO_TAPS", "TAPS_FUSE", "BNECK_FUSE", "BNECK_PROJ", "BNECK_L2", "STEM_POOL",
                       "PATCH_VIEW", "T1_BORDER") if getattr(E, s) is not True]
    assert not off, f"prpe.engine switches not at their defaults: {off}"


def pow2_ceil(v):
    c = 1.0
    while c < v:
        c *= 2.0
    return c


def check_taps(label, stage, case, taps, expect, bound):
    """Print every tap's figures, then assert: the tap set, the max|x| slots, the bounds.
    ``bound(name, e_ref) -> (limit, why)``. Returns the largest err / e_ref."""
    assert sorted(taps) == sorted(expect), (label, sorted(set(expect) ^ set(taps)))
    rows = []
    for name in expect:
        ref = case.ref[name]
        got = taps[name].value(ref.shape)
        assert got.dtype == torch.float32 and torch.isfinite(got).all(), (label, name)
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        abs_err = float((got.double() - ref).abs().max())
        loose, under = None, []
        if taps[name].amax is not None:
            tmax = got.reshape(got.shape[0], -1).abs().amax(1)
            am = taps[name].amax.cpu()
            under = [(n, float(am[n]), float(tmax[n])) for n in range(got.shape[0]) if not am[n] >= tmax[n]]
            loose = [float(am[n] / tmax[n]) for n in range(got.shape[0])]
        rows.append((name, err, abs_err, case.e_ref[name], under, loose))
        print(f"{label} {name}: err {err:.3e} e_ref {case.e_ref[name]:.3e} err/e_ref {err / case.e_ref[name]:.2f} "
              f"abs {abs_err:.3e} amax/max|t| {None if loose is None else [round(v, 4) for v in loose]}")
    for name, err, abs_err, e_ref, under, _ in rows:
        assert not under, (label, name, "max|x| slot below the tensor's maximum (frame, slot, max|t|)", under)
    for name, err, abs_err, e_ref, _, _ in rows:
        limit, why = bound(name, e_ref)
        assert limit is not None, (label, name, "no measured row for this tap", err, err / e_ref)
        assert err <= limit, (label, name, err, limit, why, err / e_ref)
        if name in FINAL_ABS:
            assert abs_err <= FINAL_ABS[name], (label, name, abs_err)
        if name in FINAL_REL:
            assert err <= FINAL_REL[name], (label, name, err)
    return max(r[1] / r[3] for r in rows)


def c_bound(stage):
    def bound(name, e_ref):
        m = RATIO.get(name)
        if m is None:
            return None, "no measured err / e_ref"
        c = min(CAP, pow2_ceil(2.0 * m))
        return c * e_ref, f"{c} x e_ref (measured err / e_ref {m}, {stage}, DESIGN.md §3)"
    return bound


def same_bits(label, a, b):
    assert sorted(a) == sorted(b), label
    for name in a:
        assert torch.equal(a[name].t, b[name].t), (label, name, "two runs differ")
        assert (a[name].amax is None) == (b[name].amax is None), (label, name)
        if a[name].amax is not None:
            assert torch.equal(a[name].amax, b[name].amax), (label, name, "two runs' max|x| slots differ")


# ------------------------------------------------------------------------------------ the trunk
def run_trunk(eng, key):
    Hh, Ww, flip, u8 = H.SIZES[key]
    x = H.frames(key)
    if u8:
        return eng.trunk_u8(H.frames_u8(key).to(DEV), FrameIngest(size=(Hh, Ww), mode="stretch", norm="unit"))
    if key == "112x112":
        xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
        m = x.abs().amax(dim=(1, 2, 3)).to(DEV)

        def fill(interior, amax):
            interior[..., :3].copy_(xd)
            if amax is not None:
                amax.copy_(m)
        return eng.trunk_from_stem_buf(eng.face_stem_buf(H.TRUNK_B), fill, Hh, Ww)
    return eng.trunk(x.to(DEV), flip_w=flip)


FUSED_BLOCKS = ["backbone.layer1.0", "backbone.layer1.1", "backbone.layer1.2", "backbone.layer2.1",
                "backbone.layer2.2", "backbone.layer2.3"]


def check_trunk_routes(label, rec, key, prec):
    """The routes the policy is there for were taken: a silent fallback fails here."""
    Hh, Ww = H.SIZES[key][:2]
    L = rec.launches
    convs = rec.convs("backbone.")
    fused = [l[1][:-len(".conv1")] for l in L if l[0] == "bottleneck"]
    assert all(c[2] == prec for c in convs), (label, [c[:3] for c in convs if c[2] != prec])
    if prec == 3:
        stem_fused = Hh % 4 == 0 and Ww % 4 == 0
        assert (("stem_maxpool",) in L) == stem_fused and (("maxpool",) in L) == (not stem_fused), label
        assert any(c[1] == "backbone.conv1" for c in convs) == (not stem_fused), label
        assert fused == FUSED_BLOCKS, (label, fused)
        assert all(c[4] is not None for c in convs), (label, "a precision-3 conv without max|x| slots")
    else:
        assert ("stem_maxpool",) not in L and ("maxpool",) in L and not fused, label
        assert all(c[4] is None for c in convs), label
    # the unfused blocks' conv2 reads the zero-bordered buffer unpadded (T1_BORDER)
    conv2 = [c for c in convs if c[1].endswith(".conv2")]
    assert len(conv2) == 16 - len(fused) and all(c[3] == 0 for c in conv2), (label, conv2)
    # block 0 of layers 2-4: the dual GEMM's second input is the ``::2`` subsample view
    dual = [c for c in convs if c[1].endswith(".conv3+downsample")]
    assert [c[5] for c in dual] == ([] if prec == 3 else [True]) + [False] * 3, (label, dual)
    return ({"backbone.conv1"} if ("stem_maxpool",) in L else set())


@pytest.mark.parametrize("policy", ["auto", 2, 3])
@pytest.mark.parametrize("key", list(H.SIZES))
def test_trunk_stage(state_dict, engine_of, monkeypatch, key, policy):
    case = H.case(state_dict, key, "trunk")
    eng = engine_of(policy)
    prec = eng.policy["trunk"]
    assert prec == (3 if policy == "auto" else policy)
    rec = Recorder(monkeypatch)
    label = f"trunk {key} policy={policy}"
    y = run_trunk(eng, key)
    torch.cuda.synchronize()
    first = rec.taps
    assert (y.amax is not None) == (prec == 3) and y.epoch == ("trunk", eng._amax_epoch.get("trunk")), label
    assert torch.equal(y.t, first[H.FEAT].t), label
    fused_away = check_trunk_routes(label, rec, key, prec)
    expect = [t for t in H.TAPS["trunk"] if t not in fused_away]
    check_taps(label, "trunk", case, first, expect, c_bound("trunk"))
    if prec == 3:            # every block output of a precision-3 trunk carries its slots
        assert all(first[t].amax is not None for t in H.TRUNK_BLOCKS), label
    rec.reset()
    run_trunk(eng, key)
    torch.cuda.synchronize()
    same_bits(label, first, rec.taps)


# ------------------------------------------------------------------------------------ the heads
def device_feat(eng, state_dict, key, x_feat):
    """The fp32 feature ``x_feat`` (the fp64 oracle's, rounded; NCHW) as the Act a trunk call of
    this engine returns: at trunk precision 3 its max|x| slots hold the feature's own per-frame
    maxima and its epoch is the trunk's current one, so feat_prec holds."""
    y = eng.trunk(H.frames(key)[:H.HEAD_B].to(DEV))
    y.t.copy_(x_feat.permute(0, 2, 3, 1).to(DEV))
    if y.amax is not None:
        y.amax.copy_(x_feat.abs().amax(dim=(1, 2, 3)).to(DEV))
    return y


def run_head(eng, stage, x):
    """``x``: the device input of the stage (an Act for the first stages, NHWC tensors else)."""
    if stage == "adaface":
        emb, norm = eng.adaface(x)
        return {"ada_face.emb": Tap(emb, "rows"), "ada_face.norm": Tap(norm, "rows")}
    with eng.prec(COMP[stage]):
        if stage == "yolo_adapter":
            out = eng.yolo_adapter(H.YOLO, x)
            return {H.YOLO + ".adapter": Tap(out.t, "nhwc")}
        if stage == "yolo_net":
            det = eng.yolo_net(H.YOLO, x, H.STRIDE)
            return {H.YOLO + ".det.box": Tap(det[:, :4], "rows"), H.YOLO + ".det.cls": Tap(det[:, 4:], "rows")}
        if stage == "vit_adapter":
            eng.vit_adapter(x)
            return {}
        return {"vit_pose.heatmaps": Tap(eng.vit_backbone(x), "rows")}


def head_input(eng, state_dict, key, stage, case):
    if stage in ("yolo_adapter", "adaface", "vit_adapter"):
        return device_feat(eng, state_dict, key, case.x)
    return case.x.permute(0, 2, 3, 1).contiguous().to(DEV)


def head_bound(stage, policy, table):
    """Precision 2 stages (and "auto"'s yolo_net): c x e_ref. Precision 0 / 4 stages: twice the
    measured err of ``table``."""
    if policy == 2 or E.AUTO_POLICY[COMP[stage]] in (2, 3):
        return c_bound(stage)

    def bound(name, e_ref):
        m = table.get(name)
        return (None if m is None else 2.0 * m), f"2 x the measured {m} ({stage}, DESIGN.md §3)"
    return bound


def first_conv(stage):
    return {"yolo_adapter": H.YOLO + ".adapter.0", "adaface": _A + ".0", "vit_adapter": _VA + ".0"}.get(stage)


def head_fused_away(rec, stage, policy):
    """vit_adapter at precision 0: .7's epilogue runs .10's tap GEMM and its own output stays in LDS."""
    if stage == "vit_adapter" and policy == "auto":
        assert any(l[1] == _VA + ".7" for l in rec.convs()), "vit_adapter .7 was not launched"
        return {_VA + ".7"}
    return set()


@pytest.mark.parametrize("policy", ["auto", 2])
@pytest.mark.parametrize("stage", H.HEAD_STAGES)
@pytest.mark.parametrize("key", H.HEAD_SIZES)
def test_head_stage(state_dict, engine_of, monkeypatch, key, stage, policy):
    case = H.case(state_dict, key, stage)
    eng = engine_of(policy)
    comp_prec = eng.policy[COMP[stage]]
    label = f"{stage} {key} policy={policy}"
    rec = Recorder(monkeypatch)
    runs = []
    for _ in range(2):
        x = head_input(eng, state_dict, key, stage, case)
        rec.reset()
        extra = run_head(eng, stage, x)
        torch.cuda.synchronize()
        runs.append((dict(rec.taps, **extra), list(rec.launches)))
    taps, launches = runs[0]
    # routes: the stage's first conv over the trunk feature at feat_prec's 3 while the trunk epoch
    # holds (policy "auto"), every conv of a precision-2 stage at 2, no conv below the stage's own
    convs = [l for l in launches if l[0] == "conv2d"]
    assert convs, label
    if first_conv(stage):
        c0 = [c for c in convs if c[1] == first_conv(stage)]
        assert len(c0) == 1 and c0[0][2] == (3 if policy == "auto" else 2), (label, c0)
        assert (c0[0][4] is not None) == (policy == "auto"), (label, "feat_prec's conv reads the trunk's slots")
    if comp_prec == 2:
        # (the IR-50 output layer's split-K GEMM is pinned to precision 0 by Engine._adaface)
        off = [c[:3] for c in convs if c[2] != 2 and c[1] != "ir50.output"]
        assert not off, (label, off)
    if stage == "adaface" and policy == "auto":
        body = [c for c in convs if ".body." in c[1] or c[1].startswith(_A)]
        assert all(c[2] in (3, 4) for c in body), (label, [c[:3] for c in body if c[2] not in (3, 4)])
    expect = [t for t in H.TAPS[stage] if t not in head_fused_away(rec, stage, policy)]
    check_taps(label, stage, case, taps, expect, head_bound(stage, policy, ERR_AUTO))
    same_bits(label, taps, runs[1][0])


def test_heads_on_a_stale_trunk_feature(state_dict, engine_of, monkeypatch):
    """A second trunk call (on frames 64 times smaller) re-zeroes the trunk pool before the heads
    run: the feature's slots now bound another tensor. feat_prec must give way to the head's own
    precision and no conv may read those slots as the feature's scale (a precision-4 AdaFace
    without slots runs precision 0)."""
    key, policy = "64x96", "auto"
    eng = engine_of(policy)
    rec = Recorder(monkeypatch)
    for stage in ("yolo_adapter", "adaface", "vit_adapter"):
        case = H.case(state_dict, key, stage)
        label = f"stale {stage} {key}"
        feat = device_feat(eng, state_dict, key, case.x)
        eng.trunk((H.frames(key)[:H.HEAD_B] / 64).to(DEV))
        assert eng.feat_prec(feat) is None
        rec.reset()
        extra = run_head(eng, stage, feat)
        torch.cuda.synchronize()
        c0 = [c for c in rec.convs() if c[1] == first_conv(stage)]
        assert len(c0) == 1 and c0[0][2] == 0 and c0[0][4] is None, (label, c0)
        expect = [t for t in H.TAPS[stage] if t not in head_fused_away(rec, stage, policy)]
        check_taps(label, stage, case, dict(rec.taps, **extra), expect, head_bound(stage, policy, ERR_STALE))
