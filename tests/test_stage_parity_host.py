"""CPU: the per-stage oracle of the engine's stage parity harness (tests/test_gpu_stage_parity.py).

oracle/model_ref.py's stage functions take ``taps``: a dict they fill with named intermediate
outputs. This module runs every stage twice from the same fp32 input, in fp64 (state dict and
input cast to double) and in fp32, and keeps per tap

    ref[tap]    the fp64 value (what the GPU is compared with),
    e_ref[tap]  max|fp32 - fp64| / max|fp64|: the fp32 oracle's own error at that tap.

A stage's GPU error is judged against e_ref, not against the 1e-3 end-to-end bars.

Stages do not chain: each is fed the fp64 output of the stage before it, rounded to fp32 (the
heads the fp64 trunk feature, yolo_net the fp64 adapter map, vit_backbone the fp64 pixel_values),
so a failure names its stage. Inside a stage the taps do chain, in the fp32 oracle as on the GPU,
which is what keeps e_ref comparable. AdaFace is one stage (adapter + IR-50): the engine has one
entry point for it (Engine.adaface), so it cannot be fed in the middle.

The cases (SIZES) are the smallest frames that reach each route of prpe/engine.py; the GPU module
says which. The trunk runs batch 3, the heads batch 2 (frames 0 and 1 of the trunk batch). Frame n
of a trunk batch is scaled by FRAME_GAIN[n], so its max|x| differs from its batch-mates' and a
per-frame max|x| slot read at the wrong index under- or over-scales visibly.

The conditions that make the GPU comparison meaningful are asserted here, where only the reference
is involved: every tap has max|fp64| > 0 and e_ref > 0, every post-ReLU / PReLU / GELU tap has at
least 10 % of its elements non-zero in every frame, and e_ref < 1e-4 (the two oracles agree; not
a bar for the GPU). Were a tap dead at one size, the seeded input is what would change (the
synthetic weights are the session's); with FRAME_GAIN and the seeds below none is.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import model_ref as R
from prpe import synth

YOLO = "yolo_face"
STRIDE = (8.0, 16.0, 32.0)
TRUNK_B, HEAD_B = 3, 2
FRAME_GAIN = (1.0, 0.5, 2.0)
U8_A, U8_B = 1.0 / 255.0, 0.0            # FrameIngest(norm="unit"): the ingest writes v * a + b

# size key -> (H, W, flip_w, uint8 source)
SIZES = {
    "64x96": (64, 96, False, False),
    "112x112": (112, 112, False, False),
    "70x54": (70, 54, False, False),
    "96x136_flip": (96, 136, True, False),
    "64x96_u8": (64, 96, False, True),
}
HEAD_SIZES = ("64x96", "70x54")
HEAD_STAGES = ("yolo_adapter", "yolo_net", "adaface", "vit_adapter", "vit_backbone")
CASES = [(k, "trunk") for k in SIZES] + [(k, s) for k in HEAD_SIZES for s in HEAD_STAGES]

_A, _M, _V = "ada_face.adapter", "ada_face.adaface_model", "vit_pose.vit_pose.backbone"
_VA = "vit_pose.adapter"
TRUNK_BLOCKS = [f"backbone.layer{li}.{b}" for li, n in enumerate((3, 4, 6, 3), 1) for b in range(n)]
# the taps of every stage, in execution order
TAPS = {
    "trunk": ["backbone.conv1", "backbone.maxpool"] + TRUNK_BLOCKS,
    "yolo_adapter": [YOLO + ".adapter"],
    "yolo_net": [f"{YOLO}.yolo.fpn.P{i}" for i in (3, 4, 5)] + [YOLO + ".yolo.head.raw", YOLO + ".det.box",
                                                                 YOLO + ".det.cls"],
    "adaface": [_A + ".0", _A + ".4", _A + ".7", _A + ".10", _M + ".input_layer"] +
               [f"{_M}.body.{i}" for i in (2, 6, 20, 23)] + [_M + ".output", "ada_face.norm", "ada_face.emb"],
    "vit_adapter": [_VA + ".0", _VA + ".4", _VA + ".7", _VA + ".10"],
    "vit_backbone": [_V + ".embeddings"] + [f"{_V}.encoder.layer.{i}" for i in (0, 5, 11)] +
                    [_V + ".layernorm", "vit_pose.heatmaps"],
}
FEAT = TRUNK_BLOCKS[-1]
# taps that are the output of a ReLU, PReLU or GELU (the liveness condition)
ACTIVATED = set(TAPS["trunk"]) | set(TAPS["adaface"][:5]) | set(TAPS["vit_adapter"]) | {_V + ".layernorm"}
# the engine's final LayerNorm launch applies the decoder's ReLU (modeling_vitpose.py:139) as well:
# the tap is compared after it, in both oracles
POST = {_V + ".layernorm": F.relu}


def frames_u8(key):
    H, W = SIZES[key][:2]
    g = torch.Generator().manual_seed(4100 + H + W)
    return torch.randint(0, 256, (TRUNK_B, H, W, 3), generator=g, dtype=torch.uint8)


def frames(key):
    """The fp32 frames [3, 3, H, W] of a size: what Engine.trunk is given (before any flip), or, for
    the uint8 case, the values the ingest is specified to write."""
    H, W, _, u8 = SIZES[key]
    if u8:
        return (frames_u8(key).float() * torch.tensor(U8_A) + U8_B).permute(0, 3, 1, 2).contiguous()
    x = synth.frames(TRUNK_B, H, W, name="stage_parity")
    return x * torch.tensor(FRAME_GAIN).view(-1, 1, 1, 1)


class Case:
    """x: the stage's fp32 input (NCHW). ref / e_ref / live: per tap, the fp64 value, the fp32
    oracle's relative error, and the smallest per-frame fraction of non-zero elements."""

    def __init__(self, x, ref, e_ref, live):
        self.x, self.ref, self.e_ref, self.live = x, ref, e_ref, live


def _run_stage(sd, stage, x):
    taps = {}
    if stage == "trunk":
        R.resnet50_trunk(sd, x, taps=taps)
    elif stage == "yolo_adapter":
        R.yolo_adapter(sd, YOLO, x, taps=taps)
    elif stage == "yolo_net":
        det = R.yolo_net(sd, YOLO, x, STRIDE, taps=taps)
        taps[YOLO + ".det.box"], taps[YOLO + ".det.cls"] = det[:, :4], det[:, 4:]
    elif stage == "adaface":
        R.adaface_branch(sd, x, taps=taps)
    elif stage == "vit_adapter":
        R.vitpose_adapter(sd, x, taps=taps)
    elif stage == "vit_backbone":
        R.vitpose_backbone(sd, x, taps=taps)
    else:
        raise KeyError(stage)
    return {k: POST[k](v) if k in POST else v for k, v in taps.items()}


_SD64, _CACHE = {}, {}


def _sd64(sd):
    if id(sd) not in _SD64:
        _SD64[id(sd)] = (sd, {k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
    return _SD64[id(sd)][1]


def _stage_input(sd, key, stage):
    """The fp32 input of a stage: frames for the trunk, else the fp64 output of the stage before
    it, rounded to fp32 (frames 0 and 1)."""
    if stage == "trunk":
        x = frames(key)
        return torch.flip(x, dims=[-1]) if SIZES[key][2] else x
    if stage in ("yolo_adapter", "adaface", "vit_adapter"):
        return case(sd, key, "trunk").ref[FEAT][:HEAD_B].float()
    if stage == "yolo_net":
        return case(sd, key, "yolo_adapter").ref[YOLO + ".adapter"].float()
    return case(sd, key, "vit_adapter").ref[_VA + ".10"].float()


def case(sd, key, stage) -> Case:
    """The Case of (size key, stage) over the state dict ``sd``, computed once per process."""
    k = (id(sd), key, stage)
    if k not in _CACHE:
        if torch.get_num_threads() > 16:
            torch.set_num_threads(16)
        x = _stage_input(sd, key, stage)
        with torch.no_grad():
            t64 = _run_stage(_sd64(sd), stage, x.double())
            t32 = _run_stage(sd, stage, x)
        assert list(t64) == list(t32) == TAPS[stage], (list(t64), TAPS[stage])
        e_ref, live = {}, {}
        for name, r in t64.items():
            assert r.dtype == torch.float64 and t32[name].dtype == torch.float32, name
            e_ref[name] = float((t32[name].double() - r).abs().max() / r.abs().max())
            live[name] = float((r.reshape(r.shape[0], -1) != 0).double().mean(1).min())
        _CACHE[k] = Case(x, t64, e_ref, live)
    return _CACHE[k]


@pytest.mark.parametrize("key,stage", CASES)
def test_oracles_agree_and_taps_are_live(state_dict, key, stage):
    c = case(state_dict, key, stage)
    assert c.x.dtype == torch.float32 and c.x.shape[0] == (TRUNK_B if stage == "trunk" else HEAD_B)
    for name in TAPS[stage]:
        amax = float(c.ref[name].abs().max())
        print(f"{key} {stage} {name}: shape {list(c.ref[name].shape)} max|fp64| {amax:.3e} "
              f"e_ref {c.e_ref[name]:.3e} live {c.live[name]:.3f}")
        assert amax > 0 and c.e_ref[name] > 0, name
        assert c.e_ref[name] < 1e-4, (name, c.e_ref[name])
        if name in ACTIVATED:
            assert c.live[name] >= 0.10, (name, c.live[name])


def test_frames_of_a_batch_have_different_maxima():
    for key, (_, _, _, u8) in SIZES.items():
        m = frames(key).abs().amax(dim=(1, 2, 3))
        if not u8:
            assert float(m[1]) < 0.6 * float(m[0]) and float(m[2]) > 1.9 * float(m[0]), (key, m)


def test_taps_change_no_result(state_dict):
    """``taps`` only records: every stage function returns the same bits with and without it."""
    feat = case(state_dict, "64x96", "trunk").ref[FEAT][:1].float()
    sd = state_dict
    with torch.no_grad():
        assert torch.equal(R.resnet50_trunk(sd, frames("64x96")[:1]), R.resnet50_trunk(sd, frames("64x96")[:1], taps={}))
        assert torch.equal(R.yolo_branch(sd, YOLO, feat, STRIDE), R.yolo_branch(sd, YOLO, feat, STRIDE, taps={}))
        assert torch.equal(R.yolo_branch(sd, YOLO, feat, STRIDE),
                           R.yolo_net(sd, YOLO, R.yolo_adapter(sd, YOLO, feat), STRIDE))
        assert torch.equal(R.adaface_branch(sd, feat)[0], R.adaface_branch(sd, feat, taps={})[0])
        pix = R.vitpose_adapter(sd, feat)
        assert torch.equal(pix, R.vitpose_adapter(sd, feat, taps={}))
        assert torch.equal(R.vitpose_backbone(sd, pix), R.vitpose_backbone(sd, pix, taps={}))
