"""Annotated frames out: skeletons, boxes and face redaction painted on the device (DESIGN.md §5n;
csrc/annotate.hip behind prpe_annotate_nv12 / prpe_annotate_u8).

    annotator = Annotator(colour_by="track", redact="unknown")
    out = tracker.from_frames_u8(nv12, ingest)             # PersonTracker, PersonRecognition or TopDownPose
    annotator(nv12, out)                                   # in place; nothing is read from the device
    encoder.submit(surface)

The frames are painted in place: a caller who needs the clean picture copies it first. Everything
the kernels read is what the pipeline left on the device; the per-person colour and the per-face
mode are formed from ``track_id`` / ``person_ident`` / the faces' ``ident`` with torch ops there.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .nv12 import NV12Frames

# Kr, Kb of the two matrices NV12Frames knows
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
COLOUR_BY = ("track", "ident", "slot")
REDACT = ("none", "unknown", "known", "all")
REDACT_MODE = {"pixelate": 1, "fill": 2}
# twelve well separated hues; persons take index id % 12
DEFAULT_PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
                   (70, 240, 240), (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (170, 110, 40))


def rgb_to_yuv(rgb, matrix="bt709", range="limited"):
    """RGB rows (0..255) -> (Y, U, V) uint8 rows by the inverse of the surface's matrix and range,
    in fp64 on the host, rounded half to even and clamped: Y = Kr R + Kg G + Kb B,
    U = (B - Y) / (2 (1 - Kb)), V = (R - Y) / (2 (1 - Kr)); full range adds 128 to U and V, limited
    range scales luma by 219/255 from 16 and chroma by 224/255 around 128."""
    if matrix not in KR_KB or range not in ("limited", "full"):
        raise ValueError(f"rgb_to_yuv: matrix {matrix!r} / range {range!r}")
    kr, kb = KR_KB[matrix]
    c = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    y = kr * c[:, 0] + (1.0 - kr - kb) * c[:, 1] + kb * c[:, 2]
    u, v = (c[:, 2] - y) / (2.0 * (1.0 - kb)), (c[:, 0] - y) / (2.0 * (1.0 - kr))
    if range == "limited":
        y, u, v = 16.0 + y * (219.0 / 255.0), u * (224.0 / 255.0), v * (224.0 / 255.0)
    return np.clip(np.rint(np.stack([y, u + 128.0, v + 128.0], 1)), 0, 255).astype(np.uint8)


class Annotator:
    """``palette_rgb``: RGB triples, a person takes ``id % len(palette_rgb)``. ``colour_by``: the id
    is the ``"track"`` id, the ``"ident"`` (the gallery label) or the list ``"slot"``; a person
    without one (no track, nobody known) takes ``unknown_rgb``. ``redact``: which faces are
    redacted -- ``"none"``, ``"unknown"`` (ident < 0), ``"known"`` or ``"all"``; ``redact_mode``:
    ``"pixelate"`` (``cell``: the smallest block side, even, 2..64) or ``"fill"`` with
    ``redact_rgb``. ``box_t``: outline thickness (0: no boxes); ``limb_r``, ``kp_r``: radii in
    pixels; ``kp_thr``: the score a keypoint needs; ``limbs``: pairs of keypoint indices.
    ``channel_order``: of uint8 frames, ``"rgb"`` or ``"bgr"``."""

    def __init__(self, palette_rgb=DEFAULT_PALETTE, colour_by="track", redact="none", redact_mode="pixelate",
                 unknown_rgb=(160, 160, 160), redact_rgb=(0, 0, 0), limbs=ops.COCO_LIMBS, box_t=2, limb_r=1, kp_r=2,
                 kp_thr=0.3, cell=8, channel_order="rgb"):
        if colour_by not in COLOUR_BY:
            raise ValueError(f"Annotator: colour_by must be one of {COLOUR_BY}, got {colour_by!r}")
        if redact not in REDACT:
            raise ValueError(f"Annotator: redact must be one of {REDACT}, got {redact!r}")
        if redact_mode not in REDACT_MODE:
            raise ValueError(f"Annotator: redact_mode must be one of {sorted(REDACT_MODE)}, got {redact_mode!r}")
        if channel_order not in ("rgb", "bgr"):
            raise ValueError(f"Annotator: channel_order {channel_order!r}: expected 'rgb' or 'bgr'")
        rows = np.asarray(list(palette_rgb) + [unknown_rgb, redact_rgb], dtype=np.int64)
        if rows.ndim != 2 or rows.shape[1] != 3 or rows.shape[0] < 3 or rows.min() < 0 or rows.max() > 255:
            raise ValueError("Annotator: palette_rgb must hold at least one RGB triple of values 0..255")
        self.rgb = rows.astype(np.uint8)
        self.n = rows.shape[0] - 2                 # person colours; n: unknown, n + 1: redaction
        self.colour_by, self.redact, self.mode = colour_by, redact, REDACT_MODE[redact_mode]
        self.limbs = tuple((int(a), int(b)) for a, b in limbs)
        self.kw = dict(box_t=int(box_t), limb_r=int(limb_r), kp_r=int(kp_r), kp_thr=float(kp_thr), cell=int(cell))
        self.channel_order = channel_order
        self._palettes, self._work = {}, {}

    # ------------------------------------------------------------------ cached device tensors
    def palette(self, frames):
        """The palette of ``frames``' pixel format: uint8 [n + 2, 4] on their device."""
        if isinstance(frames, NV12Frames):
            key = (frames.device, frames.matrix, frames.range)
            rows = lambda: rgb_to_yuv(self.rgb, frames.matrix, frames.range)
        else:
            key = (frames.device, self.channel_order)
            rows = lambda: self.rgb if self.channel_order == "rgb" else self.rgb[:, ::-1]
        if key not in self._palettes:
            host = np.zeros((self.rgb.shape[0], 4), dtype=np.uint8)
            host[:, :3] = rows()
            self._palettes[key] = torch.from_numpy(host).to(frames.device)
        return self._palettes[key]

    def workspaces(self, max_p, max_f, K, device):
        key = (device, max_p, max_f, K)
        if key not in self._work:
            self._work[key] = ops.annotate_workspaces(max_p, max_f, K, len(self.limbs), device)
        return self._work[key]

    # ------------------------------------------------------------------ the lists
    def lists(self, out):
        """(persons, faces) as ops.annotate_* take them, from a PersonTracker, PersonRecognition or
        TopDownPose output; torch ops on the device only."""
        pose = out["pose"] if "pose" in out else out
        meta = pose["crop_meta"]
        if self.colour_by == "track":
            if "track_id" not in out:
                raise ValueError("Annotator: colour_by='track' needs a PersonTracker output (no 'track_id' here)")
            ids = out["track_id"]
        elif self.colour_by == "ident":
            if "person_ident" not in out:
                raise ValueError("Annotator: colour_by='ident' needs a PersonRecognition output (no 'person_ident' here)")
            ids = out["person_ident"]
        else:
            ids = torch.arange(meta.shape[0], device=meta.device)
        colour = torch.where(ids >= 0, ids % self.n, torch.full_like(ids, self.n)).to(torch.int32)
        persons = (meta, pose["n_crops"], pose["keypoints"], colour)
        faces = None
        if self.redact != "none":
            if "faces" not in out:
                raise ValueError(f"Annotator: redact={self.redact!r} needs an output with faces (PersonRecognition, "
                                 "PersonTracker)")
            f = out["faces"]
            fm = f["crop_meta"]
            ident = f.get("ident")
            mode = torch.full((fm.shape[0],), self.mode, device=fm.device, dtype=torch.int32)
            if self.redact != "all":
                # no identities at all: every face is unknown
                known = ident >= 0 if ident is not None else torch.zeros_like(mode, dtype=torch.bool)
                mode = torch.where(known if self.redact == "known" else ~known, mode, torch.zeros_like(mode))
            faces = (fm, f["n_crops"], mode, torch.full_like(mode, self.n + 1))
        return persons, faces

    @torch.no_grad()
    def __call__(self, frames, out, coords_hw=None):
        """Paint ``out`` into ``frames`` (a prpe.NV12Frames or a uint8 tensor [B, H, W, 3]) in
        place and return them. The ``*_u8`` entry points (which take NV12 too) give windows and
        keypoints in the pixels of their source frames: painting those frames needs no scale.
        ``coords_hw`` = (H, W) names the frame size the coordinates refer to when it is another
        one (the float entry points work in the pixels of the model frames)."""
        if isinstance(frames, (list, tuple)):
            raise ValueError("Annotator: a list of frames of mixed sizes is not supported; annotate each size's batch "
                             "with its own output")
        nv = isinstance(frames, NV12Frames)
        if not nv and not (isinstance(frames, torch.Tensor) and frames.dim() == 4):
            raise ValueError("Annotator: frames must be a prpe.NV12Frames or a uint8 tensor [B, H, W, 3]")
        H, W = (frames.shape[1:] if nv else frames.shape[1:3])
        scale = (1.0, 1.0) if coords_hw is None else (W / float(coords_hw[1]), H / float(coords_hw[0]))
        persons, faces = self.lists(out)
        table, means = self.workspaces(persons[0].shape[0], faces[0].shape[0] if faces else 0, persons[2].shape[1],
                                       persons[0].device)
        call = ops.annotate_nv12 if nv else ops.annotate_u8
        return call(frames, self.palette(frames), persons=persons, faces=faces, limbs=self.limbs, table=table,
                    means=means, scale=scale, **self.kw)
