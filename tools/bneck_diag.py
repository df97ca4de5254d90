"""Diagnostic (GPU box): trunk features of the fused-bottleneck trunk vs the unfused one, and the
face-YOLO box error against the fp64 oracle on the golden frames (bs=2) under a few precision
policies, to see which component the box error comes from.

    python tools/bneck_diag.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd")]

import torch  # noqa: E402

from oracle import model_ref as R  # noqa: E402
from prpe import CombinedModel, arch, engine, synth  # noqa: E402


def main():
    torch.set_num_threads(16)
    sd = synth.make_state_dict(arch.state_dict_spec())
    x = synth.frames(2)
    sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    with torch.no_grad():
        f64 = R.resnet50_trunk(sd64, x.double())
        d64 = R.yolo_branch(sd64, "yolo_face", f64, [8.0, 16.0, 32.0])
    feats = {}
    for fuse in (True, False):
        engine.BNECK_FUSE = fuse
        m = CombinedModel(sd, device="cuda")
        feats[fuse] = m.engine.trunk(x.cuda()).t.permute(0, 3, 1, 2).cpu().double()
    print("fused vs unfused trunk: max|d|", (feats[True] - feats[False]).abs().max().item(),
          "bit-identical frac", (feats[True] == feats[False]).double().mean().item())
    engine.BNECK_FUSE = True
    for pol in ("auto", {"trunk": 2}, {"yolo_adapter": 2}, {"trunk": 2, "yolo_adapter": 2}, 2):
        m = CombinedModel(sd, device="cuda", precision=pol)
        e = m.engine
        feat = e.trunk(x.cuda())
        det = e.yolo("yolo_face", feat, [8.0, 16.0, 32.0]).cpu().double()
        f = feat.t.permute(0, 3, 1, 2).cpu().double()
        print(f"policy={pol}: feat err {((f - f64).abs().max() / f64.abs().max()).item():.3e} "
              f"box max|d| {(det[:, :4] - d64[:, :4]).abs().max().item():.3f} "
              f"cls {(det[:, 4] - d64[:, 4]).abs().max().item():.2e}")


if __name__ == "__main__":
    main()
