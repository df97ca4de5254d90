"""NV12 frames in: decoded video as the decoder leaves it.

    surface = decoder_output                       # uint8 [B, rows, pitch], one surface per frame
    nv12 = NV12Frames.from_surface(surface, 1080, 1920, matrix="bt709", range="limited")
    out = model.forward_all_u8(nv12, ingest)       # no conversion pass, no RGB copy
    rgb = nv12.to_rgb()                            # uint8 [B, 1080, 1920, 3], when RGB frames are wanted

A hardware decoder hands over a full-resolution luma plane, a half-resolution plane of interleaved
(U, V) pairs and a row pitch wider than the picture. ``NV12Frames`` holds the two planes as views
(nothing is copied) with the integer conversion table; every ``*_u8`` entry point of the package
takes one where it takes a uint8 tensor [B, Hs, Ws, 3], and the kernels convert each tap as they
gather it (csrc/nv12.hip). The conversion is one integer rule (include/prpe.h): replicated chroma,
``clamp((cy (Y - y_off) + chroma term + 128) >> 8, 0, 255)``.
"""
from __future__ import annotations

import torch

# (y_off, cy, crv, cgu, cgv, cbu): round(256 x) of the real matrices (include/prpe.h has the
# formulas; tests/test_nv12_host.py derives the table again in fp64)
COEF = {
    ("bt601", "limited"): (16, 298, 409, 100, 208, 516),
    ("bt601", "full"): (0, 256, 359, 88, 183, 454),
    ("bt709", "limited"): (16, 298, 459, 55, 136, 541),
    ("bt709", "full"): (0, 256, 403, 48, 120, 475),
}
MATRICES = ("bt601", "bt709")
RANGES = ("limited", "full")


# What the crop callers (prpe.topdown, prpe.faces) call on their source frames: the _nv12 op for an
# NV12Frames, the _u8 op with the ingest's channel order for a uint8 tensor [B, Hs, Ws, 3].
# ``ingest``: a prpe.FrameIngest (its a and b).
def crop_resize_src(frames, crop_meta, n_crops, crops, ingest):
    from . import ops
    if isinstance(frames, NV12Frames):
        return ops.crop_resize_nv12(frames, crop_meta, n_crops, crops, ingest.a, ingest.b)
    return ops.crop_resize_u8(frames, crop_meta, n_crops, crops, ingest.a, ingest.b, ingest.swap_rb)


def roi_resize_src(frames, crop_meta, n_crops, y, ingest, y_amax=None):
    from . import ops
    if isinstance(frames, NV12Frames):
        return ops.roi_resize_nv12(frames, crop_meta, n_crops, y, ingest.a, ingest.b, y_amax=y_amax)
    return ops.roi_resize_u8(frames, crop_meta, n_crops, y, ingest.a, ingest.b, ingest.swap_rb, y_amax=y_amax)


def roi_warp_src(frames, crop_meta, n_crops, warp, y, ingest, y_amax=None):
    from . import ops
    if isinstance(frames, NV12Frames):
        return ops.roi_warp_nv12(frames, crop_meta, n_crops, warp, y, ingest.a, ingest.b, y_amax=y_amax)
    return ops.roi_warp_u8(frames, crop_meta, n_crops, warp, y, ingest.a, ingest.b, ingest.swap_rb, y_amax=y_amax)


class NV12Frames:
    """``y``: uint8 device tensor [B, Hs, Ws], last stride 1 (the row stride is the decoder's pitch).
    ``uv``: uint8 [B, ceil(Hs/2), ceil(Ws/2), 2] = (U, V) on the same device, last strides (2, 1),
    even row and frame strides and an even address (a pair is one 16-bit load). ``matrix``: "bt601"
    or "bt709"; ``range``: "limited" (16..235) or "full". Anything else raises ``ValueError``."""

    def __init__(self, y, uv, matrix="bt709", range="limited"):
        if matrix not in MATRICES:
            raise ValueError(f"matrix {matrix!r}: expected one of {MATRICES}")
        if range not in RANGES:
            raise ValueError(f"range {range!r}: expected one of {RANGES}")
        for name, t in (("y", y), ("uv", uv)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
                raise ValueError(f"NV12Frames: {name} must be a uint8 tensor, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)}")
        if y.dim() != 3 or y.numel() == 0:
            raise ValueError(f"NV12Frames: y must be [B, Hs, Ws], got {list(y.shape)}")
        B, Hs, Ws = y.shape
        want = (B, (Hs + 1) // 2, (Ws + 1) // 2, 2)
        if tuple(uv.shape) != want:
            raise ValueError(f"NV12Frames: uv must be {list(want)} for y {list(y.shape)}, got {list(uv.shape)}")
        if uv.device != y.device:
            raise ValueError(f"NV12Frames: y is on {y.device}, uv on {uv.device}")
        if y.stride(2) != 1 or y.stride(1) < Ws:
            raise ValueError(f"NV12Frames: y must have element stride 1 along a row and a pitch of at least {Ws}, "
                             f"got strides {list(y.stride())}")
        if uv.stride(3) != 1 or uv.stride(2) != 2 or uv.stride(1) < want[2] * 2 or uv.stride(1) % 2 or \
                uv.stride(0) % 2:
            raise ValueError(f"NV12Frames: uv must hold contiguous (U, V) pairs (strides (.., .., 2, 1)) with even row "
                             f"and frame strides and a pitch of at least {want[2] * 2}, got strides {list(uv.stride())}")
        if uv.data_ptr() % 2:
            raise ValueError("NV12Frames: uv must start at an even address")
        self.y, self.uv = y, uv
        self.matrix, self.range = matrix, range
        self.coef = COEF[(matrix, range)]

    @classmethod
    def from_surface(cls, surface, height, width, uv_row=None, **kw):
        """The two views of one decoder surface ``surface`` [B, rows, pitch] uint8: luma in rows
        [0, height), chroma pairs from row ``uv_row`` on (default ``height``; a decoder that aligns
        the luma rows says where they end), both ``width`` wide at the surface's pitch, which must
        be even. Nothing is copied."""
        if not isinstance(surface, torch.Tensor) or surface.dtype != torch.uint8 or surface.dim() != 3:
            raise ValueError("from_surface: surface must be a uint8 tensor [B, rows, pitch], got "
                             f"{getattr(surface, 'dtype', type(surface).__name__)} "
                             f"{list(getattr(surface, 'shape', []))}")
        height, width = int(height), int(width)
        uv_row = height if uv_row is None else int(uv_row)
        B, rows, pitch = surface.shape
        hc, wc = (height + 1) // 2, (width + 1) // 2
        if height < 1 or width < 1 or B < 1:
            raise ValueError(f"from_surface: {B} frames of {height} x {width}")
        if surface.stride(2) != 1 or pitch % 2 or surface.stride(1) % 2 or surface.stride(0) % 2:
            raise ValueError(f"from_surface: the pitch must be even and the bytes of a row contiguous, got shape "
                             f"{list(surface.shape)} strides {list(surface.stride())}")
        if uv_row < height:
            raise ValueError(f"from_surface: uv_row {uv_row} lies inside the {height} luma rows")
        if pitch < 2 * wc or uv_row + hc > rows:
            raise ValueError(f"from_surface: a surface of {rows} rows x {pitch} bytes does not hold {height} luma rows "
                             f"and {hc} chroma rows from row {uv_row} at width {width}")
        y = surface[:, :height, :width]
        uv = surface[:, uv_row:uv_row + hc, :2 * wc].unflatten(2, (wc, 2))
        return cls(y, uv, **kw)

    @property
    def shape(self):
        """(B, Hs, Ws)."""
        return tuple(self.y.shape)

    @property
    def device(self):
        return self.y.device

    @property
    def is_cuda(self):
        return self.y.is_cuda

    def to_rgb(self, channel_order="rgb", out=None):
        """The frames converted: uint8 [B, Hs, Ws, 3] in ``channel_order`` (prpe_nv12_to_rgb), into
        ``out`` when given (any row and frame strides, 3 contiguous bytes per pixel)."""
        from . import ops
        if channel_order not in ("rgb", "bgr"):
            raise ValueError(f"channel_order {channel_order!r}: expected 'rgb' or 'bgr'")
        if out is None:
            out = torch.empty(self.shape + (3,), dtype=torch.uint8, device=self.device)
        return ops.nv12_to_rgb(self, out, swap_rb=channel_order == "bgr")

    def __repr__(self):
        B, Hs, Ws = self.shape
        return (f"NV12Frames({B} x {Hs} x {Ws}, pitch {self.y.stride(1)}, {self.matrix} {self.range}, "
                f"{self.device})")
