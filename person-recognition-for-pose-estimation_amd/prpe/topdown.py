"""Top-down pose on the device: person boxes -> ViTPose crops -> one skeleton per person.

    pose = TopDownPose(model)
    out = pose(frames)                   # [B,3,H,W] float32 device frames; no host read
    people = pose.results(out)           # the one host read: per frame, a list of persons

Stages: the trunk once, the person YOLO head, padded NMS, prpe_crop_select (the
crop list), prpe_crop_resize (bilinear crops straight into the patch embedding's zero-bordered
NHWC4 buffer), the ViTPose backbone, soft-argmax, prpe_crop_keypoints (back to frame pixels).
The reference has no runnable crop stage; the window and resample semantics are the ones
include/prpe.h states (grid_sample bilinear / zeros / align_corners=False on a 3:4 window).
"""
from __future__ import annotations

import torch

from . import arch, nv12, ops
from .postproc import non_max_suppression_padded


class TopDownPose:
    """``model``: a CombinedModel. ``max_crops`` (default B * max_per_frame) is the capacity of the
    crop list, ``box_scale`` = (x, y) detector units -> frame pixels (default: frame size over the
    YOLO adapter's output size, arch.YOLO_IMG). ``compact=False``: no host read at all, ViTPose
    runs on every one of the max_crops slots (empty slots are zero crops; their keypoints are
    zeroed). ``compact=True``: ONE host read, of n_crops -- the only synchronisation -- and
    ViTPose runs on the first n slots. Frames and crops are batch-independent, so both modes give
    the same bits in keypoints[:n]."""

    def __init__(self, model, max_per_frame=8, max_crops=None, score_thr=0.25, pad=1.25, min_size=4.0,
                 box_scale=None, branch="yolo_person", compact=False):
        if branch not in ("yolo_person", "yolo_face"):
            raise ValueError(f"branch {branch!r}: expected 'yolo_person' or 'yolo_face'")
        if max_per_frame < 1 or (max_crops is not None and max_crops < 1):
            raise ValueError("max_per_frame and max_crops must be at least 1")
        self.model = model
        self.max_per_frame, self.max_crops = int(max_per_frame), max_crops
        self.score_thr, self.pad, self.min_size = float(score_thr), float(pad), float(min_size)
        self.box_scale, self.branch, self.compact = box_scale, branch, bool(compact)

    @torch.no_grad()
    def __call__(self, frames):
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        e = m.engine
        det = e.yolo(self.branch, e.trunk(x), m._stride(getattr(m, self.branch)))
        dets, counts = non_max_suppression_padded(det)
        return self.from_detections(x, dets, counts)

    @torch.no_grad()
    def from_detections(self, frames, dets, counts):
        """Enter after NMS: dets [B, max_det, 6] (x1, y1, x2, y2, score, class; rows in descending
        score order) and counts [B] int32, e.g. from another detector."""
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        B, _, H, W = x.shape
        scale = self.box_scale
        if scale is None:
            scale = (W / arch.YOLO_IMG[1], H / arch.YOLO_IMG[0])
        return self._crops_to_keypoints(B, (H, W), dets, counts, scale,
                                        lambda meta, n_crops, buf: ops.crop_resize(x, meta, n_crops, buf))

    @torch.no_grad()
    def from_frames_u8(self, frames_u8, ingest=None):
        """uint8 source frames [B, Hs, Ws, 3] on the device (any strides) -> the same output, with
        detections, windows and keypoints in SOURCE pixels: ``ingest`` (a prpe.FrameIngest) resizes
        the frames for the trunk and the person head, the boxes go back to source pixels on the
        device, and the crops are resampled from the source frames themselves
        (prpe_crop_resize_u8, with the ingest's a, b and channel order), which hold 2-3x the
        pixels per person of the model frame. ``dets`` in the output are in source pixels."""
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest)
        m._sync_weights()
        e = m.engine
        det = e.yolo(self.branch, e.trunk_u8(frames_u8, ingest), m._stride(getattr(m, self.branch)))
        dets, counts = non_max_suppression_padded(det)
        # detector units -> model-frame pixels -> source pixels; rows past counts[b] may hold anything
        H, W = ingest.size
        scale = self.box_scale
        if scale is None:
            scale = (W / arch.YOLO_IMG[1], H / arch.YOLO_IMG[0])
        elif isinstance(scale, (int, float)):
            scale = (scale, scale)
        sx, sy = (float(v) for v in scale)
        Hs, Ws = frames_u8.shape[1:3]
        boxes = dets[..., :4].clone()
        boxes[..., 0::2] *= sx
        boxes[..., 1::2] *= sy
        dets = torch.cat([ingest.to_source(boxes, Hs, Ws), dets[..., 4:]], 2)
        return self.from_detections_u8(frames_u8, dets, counts, ingest)

    @torch.no_grad()
    def from_detections_u8(self, frames_u8, dets, counts, ingest=None):
        """Enter after NMS with uint8 source frames: ``dets`` [B, max_det, 6] in SOURCE pixels
        (``box_scale`` is not applied) and counts [B] int32. Only the ingest's a, b and channel
        order are used (the crops come from the source frames, not from the model frame)."""
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest)
        m._sync_weights()
        B, Hs, Ws = frames_u8.shape[:3]
        return self._crops_to_keypoints(
            B, (Hs, Ws), dets, counts, 1.0,
            lambda meta, n_crops, buf: nv12.crop_resize_src(frames_u8, meta, n_crops, buf, ingest))

    def _crops_to_keypoints(self, B, frame_hw, dets, counts, scale, resize):
        """crop list -> ``resize(meta, n_crops, buf)`` fills the crop buffer -> ViTPose -> keypoints
        in the pixels of the frames the windows refer to."""
        e = self.model.engine
        if dets.dim() != 3 or dets.shape[0] != B or counts.shape != (B,):
            raise ValueError(f"dets [B, max_det, 6] and counts [B] must match the {B} frames")
        cap = int(self.max_crops) if self.max_crops is not None else B * self.max_per_frame
        if isinstance(scale, (int, float)):
            scale = (scale, scale)
        dev = dets.device
        meta = torch.empty(cap, ops.CROP_META_COLS, device=dev, dtype=torch.float32)
        n_crops = torch.empty(1, device=dev, dtype=torch.int32)
        status = torch.empty(1, device=dev, dtype=torch.int32)
        kpts = torch.empty(cap, arch.NUM_KEYPOINTS, 3, device=dev, dtype=torch.float32)
        ops.crop_select(dets, counts, frame_hw, crop_meta=meta, n_crops=n_crops, status=status,
                        score_thr=self.score_thr, max_per_frame=self.max_per_frame, min_size=self.min_size,
                        box_scale=scale, pad=self.pad)
        buf = e.crop_pix4(cap)
        resize(meta, n_crops, buf)
        n = cap
        if self.compact:
            n = int(n_crops.item())                # the only host read (and synchronisation)
        if n == 0:
            kpts.zero_()
        else:
            with e.prec("vit"):
                heat = e.vit_backbone(e.pix4_interior(buf[:n]))
            coords, scores = ops.softargmax(heat)
            ops.crop_keypoints(coords, scores, meta, n_crops, kpts)
        return {"dets": dets, "counts": counts, "crop_meta": meta, "n_crops": n_crops, "status": status,
                "keypoints": kpts}

    @staticmethod
    def results(out):
        """Host view of one call's output (one device-to-host read): per frame, a list of
        ``{"box": [x0, y0, x1, y1] (the crop window in frame pixels), "score", "keypoints"
        [17, 3] = (x, y, score), "row": its row in dets[frame]}`` in detection order."""
        cols = ops.CROP_META_COLS
        both = torch.cat([out["crop_meta"], out["keypoints"].flatten(1)], 1).cpu()      # the one read
        meta, kp = both[:, :cols], both[:, cols:].reshape(-1, arch.NUM_KEYPOINTS, 3)
        frame, row = (meta[:, c].contiguous().view(torch.int32) for c in (0, 1))
        people = [[] for _ in range(out["counts"].shape[0])]
        for i in range(int((frame >= 0).sum())):   # filled slots come first; the others hold frame -1
            x0, y0, w, h, score = (float(v) for v in meta[i, 2:7])
            people[int(frame[i])].append({"box": [x0, y0, x0 + w, y0 + h], "score": score, "keypoints": kp[i],
                                          "row": int(row[i])})
        return people
