"""uint8 frames in: the geometry and normalisation of prpe_frame_ingest.

    ingest = FrameIngest(size=(640, 640), mode="letterbox", norm="unit", channel_order="bgr")
    out = model.forward_all_u8(frames_u8, ingest)        # uint8 [B, Hs, Ws, 3] device frames
    boxes_src = ingest.to_source(boxes_model, Hs, Ws)    # detections back in source pixels

The kernel resizes, pads, reorders the channels and normalises in one pass into the stem's buffer;
this class only computes what it is told: the region of the model frame the source lands in and
the per-channel affine y = raw * a + b on the raw 0..255 values. Semantics (include/prpe.h):
half-pixel-centre bilinear, no antialias -- F.interpolate(bilinear, align_corners=False), not
cv2's uint8 fixed point.
"""
from __future__ import annotations

import torch

# A.Normalize(mean, std, max_pixel_value=255): (raw / 255 - mean) / std = raw * a + b
_NORMS = {
    "unit": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),                       # object_detection/datamodule.py:95-99
    "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),       # pose_estimation/datamodule.py:389
    "half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),                       # face_recognition/datamodule.py:170
}


def _fp32(v):
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


class FrameIngest:
    """``size`` = (H, W) of the model frame. ``mode``: "stretch" resizes the source to all of it,
    "letterbox" keeps the aspect ratio in a centred region and fills the rest with ``fill`` (raw
    units, one value or three). ``norm``: "unit" (raw / 255), "imagenet", "half" ((raw / 255 - 0.5)
    / 0.5) or a pair (a, b) of 3 floats each; a and b are rounded to fp32 here, once, and are the
    values the kernel multiplies and adds. ``channel_order``: of the SOURCE; the model sees RGB,
    and a, b, fill are in the model's (output) channel order. ``antialias``: every axis that
    shrinks is filtered with torch's triangle filter (F.interpolate(..., antialias=True)) instead
    of being point-sampled: prpe_frame_ingest_multi with filter 1, for camera
    resolutions far above the model frame; it applies to the whole-frame ingest only."""

    def __init__(self, size=(640, 640), mode="letterbox", norm="unit", channel_order="rgb", fill=114,
                 antialias=False):
        H, W = (int(v) for v in size)
        if H < 1 or W < 1:
            raise ValueError(f"size {size!r}: expected (H, W), both at least 1")
        if mode not in ("letterbox", "stretch"):
            raise ValueError(f"mode {mode!r}: expected 'letterbox' or 'stretch'")
        if channel_order not in ("rgb", "bgr"):
            raise ValueError(f"channel_order {channel_order!r}: expected 'rgb' or 'bgr'")
        if isinstance(norm, str):
            if norm not in _NORMS:
                raise ValueError(f"norm {norm!r}: expected one of {sorted(_NORMS)} or a pair (a, b)")
            mean, std = _NORMS[norm]
            a = [1.0 / (255.0 * s) for s in std]
            b = [-m / s for m, s in zip(mean, std)]
        else:
            a, b = ([float(v) for v in t] for t in norm)
            if len(a) != 3 or len(b) != 3:
                raise ValueError("norm: a pair (a, b) of 3 floats each")
        fill = [float(fill)] * 3 if isinstance(fill, (int, float)) else [float(v) for v in fill]
        if len(fill) != 3:
            raise ValueError("fill: one value or 3 (raw 0..255 units)")
        self.size, self.mode, self.channel_order = (H, W), mode, channel_order
        self.a, self.b, self.fill = (tuple(_fp32(v) for v in t) for t in (a, b, fill))
        self.antialias = bool(antialias)

    @property
    def swap_rb(self) -> bool:
        return self.channel_order == "bgr"

    def geometry(self, Hs, Ws):
        """(top, left, nh, nw): the region of the model frame a Hs x Ws source is resized into."""
        H, W = self.size
        Hs, Ws = int(Hs), int(Ws)
        if Hs < 1 or Ws < 1:
            raise ValueError(f"source {Hs} x {Ws}: both sides must be at least 1")
        if self.mode == "stretch":
            return 0, 0, H, W
        s = min(H / Hs, W / Ws)
        nh = min(max(int(Hs * s + 0.5), 1), H)
        nw = min(max(int(Ws * s + 0.5), 1), W)
        return (H - nh) // 2, (W - nw) // 2, nh, nw

    def geometry_batch(self, sizes):
        """``geometry`` of every (Hs, Ws) of ``sizes`` (a sequence, or a [B, 2] tensor): an int32
        host tensor [B, 4] of (top, left, nh, nw) rows, what ``ops.frame_ingest_multi`` takes."""
        sizes = sizes.tolist() if isinstance(sizes, torch.Tensor) else [tuple(s) for s in sizes]
        if not sizes or any(len(s) != 2 for s in sizes):
            raise ValueError("sizes: a non-empty sequence of (Hs, Ws), or a [B, 2] tensor")
        return torch.tensor([self.geometry(*s) for s in sizes], dtype=torch.int32)

    def _map(self, p, Hs, Ws, inverse):
        if p.shape[-1] not in (2, 4):
            raise ValueError("expected points [..., 2] = (x, y) or boxes [..., 4] = (x1, y1, x2, y2), got "
                             f"{list(p.shape)}")
        if Ws is None:                          # Hs holds the sizes of the B frames: p[n] is mapped by frame n's
            g = self.geometry_batch(Hs).to(torch.float64)
            sizes = torch.as_tensor(Hs.tolist() if isinstance(Hs, torch.Tensor) else [tuple(s) for s in Hs],
                                    dtype=torch.float64)
            if p.dim() < 2 or p.shape[0] != g.shape[0]:
                raise ValueError(f"{g.shape[0]} sizes need points or boxes [{g.shape[0]}, ..., 2|4], got "
                                 f"{list(p.shape)}")
            # [B, 1, ..., 1] columns on p's device: the geometry comes from the host, p is never read back
            col = lambda v: v.to(device=p.device, dtype=p.dtype).reshape([-1] + [1] * (p.dim() - 1))
            offs, scs = (col(g[:, 1]), col(g[:, 0])), (col(sizes[:, 1] / g[:, 3]), col(sizes[:, 0] / g[:, 2]))
        else:
            top, left, nh, nw = self.geometry(Hs, Ws)
            offs, scs = (left, top), (Ws / nw, Hs / nh)
        out = torch.empty_like(p)
        for c in (0, 1):                                                # x columns, then y columns
            v = p[..., c::2]
            out[..., c::2] = v / scs[c] + offs[c] if inverse else (v - offs[c]) * scs[c]
        return out

    def to_source(self, p, Hs, Ws=None):
        """Model-frame points [..., 2] or boxes [..., 4] (pixel-edge coordinates: the left edge of
        pixel 0 is x = 0) -> source pixels: x_src = (x - left) * Ws / nw, y likewise. Elementwise
        torch ops on ``p``'s device; nothing is read back. ``to_source(p, sizes)``, with ``sizes``
        a sequence of B (Hs, Ws) or a [B, 2] tensor in place of ``Hs, Ws``: ``p`` is
        [B, ..., 2|4] and ``p[n]`` is mapped with frame n's geometry."""
        return self._map(p, Hs, Ws, False)

    def to_model(self, p, Hs, Ws=None):
        """The inverse of ``to_source``: x = x_src / (Ws / nw) + left."""
        return self._map(p, Hs, Ws, True)

    def __repr__(self):
        return (f"FrameIngest(size={self.size}, mode={self.mode!r}, a={self.a}, b={self.b}, "
                f"channel_order={self.channel_order!r}, fill={self.fill}"
                f"{', antialias=True' if self.antialias else ''})")
