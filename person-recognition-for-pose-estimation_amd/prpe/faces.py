"""Per-face identification on the device, and identities joined to skeletons (DESIGN.md §5e;
csrc/roi.hip behind prpe_roi_select / prpe_roi_resize / prpe_face_person_match).

    faces = FaceCrops(model, gallery)
    faces.enrol(portraits, labels)           # one face per frame -> the gallery
    out = faces(frames)                      # [B,3,H,W] float32 device frames; no host read
    people = PersonRecognition(model, gallery)
    persons = people.results(people(frames)) # per frame: box, keypoints, ident, ...

``FaceCrops``: the trunk once, the face YOLO head, padded NMS, prpe_roi_select (square windows),
prpe_roi_resize (112 x 112 bilinear crops straight into a stem buffer, with the per-crop max|x|
the precision-3 stem needs), the trunk again on the crops, AdaFace, the gallery. The face branch
is trained on 112 x 112 face images through the shared trunk
(training/lightning/face_recognition/datamodule.py:41, scripts/modify_models.py:225-297), so this
is the route its embedding is meant for; ``FaceIdentifier`` embeds the whole frame.
``PersonRecognition``: one trunk, both heads, top-down pose and per-face identities, then
prpe_face_person_match gives every skeleton the identity of the face at its head.
"""
from __future__ import annotations

import torch

from . import arch, nv12, ops
from .gallery import FaceGallery
from .postproc import non_max_suppression_padded
from .topdown import TopDownPose

EMB_DIM = 512


def _scale_xy(scale, frame_hw):
    """``box_scale`` as (x, y): None -> frame size over the YOLO adapter's output size."""
    if scale is None:
        return frame_hw[1] / arch.YOLO_IMG[1], frame_hw[0] / arch.YOLO_IMG[0]
    if isinstance(scale, (int, float)):
        return float(scale), float(scale)
    sx, sy = scale
    return float(sx), float(sy)


def _to_source(dets, scale, ingest, src_hw):
    """Detector units -> model-frame pixels -> source pixels (rows past counts[b] may hold anything)."""
    boxes = dets[..., :4].clone()
    boxes[..., 0::2] *= scale[0]
    boxes[..., 1::2] *= scale[1]
    return torch.cat([ingest.to_source(boxes, *src_hw), dets[..., 4:]], 2)


class FaceCrops:
    """``model``: a CombinedModel; ``gallery``: a 512-d FaceGallery or None (embeddings only).
    ``max_crops`` (default B * max_per_frame) is the capacity of the crop list, ``box_scale`` =
    (x, y) detector units -> frame pixels (default: frame size over arch.YOLO_IMG), ``pad`` grows
    the square window about the box centre, ``threshold`` is the gallery's rejection bar.
    ``compact=False``: no host read at all, the trunk and AdaFace run on every one of the max_crops
    slots (empty slots are zero crops; their outputs are masked on the device). ``compact=True``:
    ONE host read, of n_crops, and they run on the first n slots. Crops are batch-independent, so
    both modes give the same bits in [:n]."""

    def __init__(self, model, gallery=None, max_per_frame=8, max_crops=None, score_thr=0.25, pad=1.25, min_size=4.0,
                 box_scale=None, threshold=0.3, compact=False):
        if max_per_frame < 1 or (max_crops is not None and max_crops < 1):
            raise ValueError("max_per_frame and max_crops must be at least 1")
        if gallery is not None and not isinstance(gallery, FaceGallery):
            raise ValueError(f"FaceCrops: gallery must be a prpe.FaceGallery, got {type(gallery).__name__}")
        if gallery is not None and gallery.dim != EMB_DIM:
            raise ValueError(f"FaceCrops: the AdaFace embedding is {EMB_DIM}-d, the gallery holds {gallery.dim}")
        if not float(pad) > 0.0:
            raise ValueError(f"FaceCrops: pad must be positive, got {pad}")
        self.model, self.gallery = model, gallery
        self.max_per_frame, self.max_crops = int(max_per_frame), max_crops
        self.score_thr, self.pad, self.min_size = float(score_thr), float(pad), float(min_size)
        self.box_scale, self.threshold, self.compact = box_scale, float(threshold), bool(compact)

    # ------------------------------------------------------------------ entry points
    @torch.no_grad()
    def __call__(self, frames):
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        e = m.engine
        det = e.yolo("yolo_face", e.trunk(x), m._stride(m.yolo_face))
        dets, counts = non_max_suppression_padded(det)
        return self.from_detections(x, dets, counts)

    @torch.no_grad()
    def from_detections(self, frames, dets, counts):
        """Enter after NMS: dets [B, max_det, 6] (x1, y1, x2, y2, score, class; rows in descending
        score order) and counts [B] int32, e.g. from another face detector."""
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        B, _, H, W = x.shape
        return self._crops_to_identities(
            B, (H, W), dets, counts, _scale_xy(self.box_scale, (H, W)),
            lambda meta, n_crops, y, amax: ops.roi_resize(x, meta, n_crops, y, y_amax=amax))

    @torch.no_grad()
    def from_frames_u8(self, frames_u8, ingest=None):
        """uint8 source frames [B, Hs, Ws, 3] on the device (any strides) -> the same output with
        detections and windows in SOURCE pixels: ``ingest`` (a prpe.FrameIngest) resizes the frames
        for the trunk and the face head, the boxes go back to source pixels on the device, and the
        crops are resampled from the source frames (prpe_roi_resize_u8 with the ingest's a, b and
        channel order)."""
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest)
        m._sync_weights()
        e = m.engine
        det = e.yolo("yolo_face", e.trunk_u8(frames_u8, ingest), m._stride(m.yolo_face))
        dets, counts = non_max_suppression_padded(det)
        dets = _to_source(dets, _scale_xy(self.box_scale, ingest.size), ingest, frames_u8.shape[1:3])
        return self.from_detections_u8(frames_u8, dets, counts, ingest)

    @torch.no_grad()
    def from_detections_u8(self, frames_u8, dets, counts, ingest=None):
        """Enter after NMS with uint8 source frames: ``dets`` [B, max_det, 6] in SOURCE pixels
        (``box_scale`` is not applied) and counts [B] int32. Only the ingest's a, b and channel
        order are used."""
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest)
        m._sync_weights()
        B, Hs, Ws = frames_u8.shape[:3]
        return self._crops_to_identities(
            B, (Hs, Ws), dets, counts, (1.0, 1.0),
            lambda meta, n_crops, y, amax: nv12.roi_resize_src(frames_u8, meta, n_crops, y, ingest, y_amax=amax))

    # ------------------------------------------------------------------ the stage
    def _crops_to_identities(self, B, frame_hw, dets, counts, scale, resize, max_per_frame=None, identify=True,
                             warp=None):
        """crop list -> ``resize(meta, n_crops, y, amax)`` fills the stem buffer inside the trunk's
        scope -> trunk at 112 x 112 -> AdaFace -> the gallery. ``warp`` (PersonRecognition's aligned
        crops): ``warp(meta, n_crops)`` gives the list's warp rows [cap, 8] once the list is made,
        ``resize`` takes their first n as a fifth argument, and the output gains ``"warp"``."""
        e = self.model.engine
        if dets.dim() != 3 or dets.shape[0] != B or counts.shape != (B,):
            raise ValueError(f"dets [B, max_det, 6] and counts [B] must match the {B} frames")
        per_frame = self.max_per_frame if max_per_frame is None else max_per_frame
        cap = int(self.max_crops) if self.max_crops is not None and max_per_frame is None else B * per_frame
        dev = dets.device
        meta = torch.empty(cap, ops.CROP_META_COLS, device=dev, dtype=torch.float32)
        n_crops = torch.empty(1, device=dev, dtype=torch.int32)
        status = torch.empty(1, device=dev, dtype=torch.int32)
        ops.roi_select(dets, counts, frame_hw, arch.FACE_IMG, crop_meta=meta, n_crops=n_crops, status=status,
                       score_thr=self.score_thr, max_per_frame=per_frame, min_size=self.min_size, box_scale=scale,
                       pad=self.pad)
        rows = None if warp is None else warp(meta, n_crops)
        emb = torch.zeros(cap, EMB_DIM, device=dev, dtype=torch.float32)
        norms = torch.zeros(cap, device=dev, dtype=torch.float32)
        ident = torch.full((cap,), -1, device=dev, dtype=torch.int64)
        score = torch.full((cap,), float("-inf"), device=dev, dtype=torch.float32)
        n = cap
        if self.compact:
            n = int(n_crops.item())                # the only host read (and synchronisation)
        if n > 0:
            H0, W0 = arch.FACE_IMG
            buf = e.face_stem_buf(cap)[:n]
            if rows is None:
                feat = e.trunk_from_stem_buf(buf, lambda y, amax: resize(meta[:n], n_crops, y, amax), H0, W0)
            else:
                feat = e.trunk_from_stem_buf(buf, lambda y, amax: resize(meta[:n], n_crops, y, amax, rows[:n]), H0, W0)
            en, nn = e.adaface(feat)
            live = torch.arange(n, device=dev, dtype=torch.int32) < n_crops      # slots below n_crops, on the device
            emb[:n] = torch.where(live[:, None], en, emb[:n])
            norms[:n] = torch.where(live, nn.view(n), norms[:n])
            if identify and self.gallery is not None and len(self.gallery) > 0:
                idn, sc = self.gallery.identify(emb[:n], self.threshold)
                ident[:n] = torch.where(live, idn, ident[:n])
                score[:n] = torch.where(live, sc, score[:n])
        out = {"dets": dets, "counts": counts, "crop_meta": meta, "n_crops": n_crops, "status": status,
               "embeddings": emb, "norms": norms, "ident": ident, "score": score}
        if rows is not None:
            out["warp"] = rows
        return out

    # ------------------------------------------------------------------ enrolment (one host read)
    def _enrol(self, out, labels, B):
        if self.gallery is None:
            raise ValueError("FaceCrops.enrol: no gallery to enrol into")
        lab = torch.as_tensor(labels, dtype=torch.int64).reshape(-1)
        if lab.numel() != B:
            raise ValueError(f"FaceCrops.enrol: {B} frames with {lab.numel()} labels")
        frame = out["crop_meta"][:, 0].contiguous().view(torch.int32).cpu()       # the one read
        n = int((frame >= 0).sum())                # filled slots come first
        found = [int(f) for f in frame[:n]]
        if n:
            self.gallery.add(out["embeddings"][:n], lab.cpu()[found])
        return [b for b in range(B) if b not in set(found)]

    @torch.no_grad()
    def enrol(self, frames, labels):
        """The best face of every frame (``max_per_frame`` = 1) goes into the gallery with
        ``labels[frame]``. Not the live path: one host read. Returns the indices of the frames that
        contributed no face (no box at or above ``score_thr`` and ``min_size``)."""
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        e = m.engine
        det = e.yolo("yolo_face", e.trunk(x), m._stride(m.yolo_face))
        dets, counts = non_max_suppression_padded(det)
        return self.enrol_detections(x, dets, counts, labels)

    @torch.no_grad()
    def enrol_detections(self, frames, dets, counts, labels):
        """``enrol`` entered after NMS (``from_detections``' arguments)."""
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        B, _, H, W = x.shape
        out = self._crops_to_identities(
            B, (H, W), dets, counts, _scale_xy(self.box_scale, (H, W)),
            lambda meta, n_crops, y, amax: ops.roi_resize(x, meta, n_crops, y, y_amax=amax),
            max_per_frame=1, identify=False)
        return self._enrol(out, labels, B)

    @torch.no_grad()
    def enrol_u8(self, frames_u8, labels, ingest=None):
        """``enrol`` on uint8 source frames [B, Hs, Ws, 3] (``from_frames_u8``)."""
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest)
        m._sync_weights()
        e = m.engine
        det = e.yolo("yolo_face", e.trunk_u8(frames_u8, ingest), m._stride(m.yolo_face))
        dets, counts = non_max_suppression_padded(det)
        dets = _to_source(dets, _scale_xy(self.box_scale, ingest.size), ingest, frames_u8.shape[1:3])
        B, Hs, Ws = frames_u8.shape[:3]
        out = self._crops_to_identities(
            B, (Hs, Ws), dets, counts, (1.0, 1.0),
            lambda meta, n_crops, y, amax: nv12.roi_resize_src(frames_u8, meta, n_crops, y, ingest, y_amax=amax),
            max_per_frame=1, identify=False)
        return self._enrol(out, labels, B)

    @staticmethod
    def results(out):
        """Host view of one call's output (one device-to-host read): per frame, a list of
        ``{"box": [x0, y0, x1, y1] (the crop window in frame pixels), "score" (the detector's),
        "row": its row in dets[frame], "slot", "ident" (-1: nobody), "ident_score"}`` in
        detection order."""
        cols = ops.CROP_META_COLS
        both = torch.cat([out["crop_meta"].view(torch.int32), out["score"].view(torch.int32)[:, None],
                          out["ident"].view(torch.int32).view(-1, 2)], 1).cpu()                   # the one read
        meta = both[:, :cols].contiguous().view(torch.float32)
        score = both[:, cols].contiguous().view(torch.float32)
        ident = both[:, cols + 1:].contiguous().view(torch.int64).view(-1)
        frame, row = both[:, 0], both[:, 1]
        faces = [[] for _ in range(out["counts"].shape[0])]
        for i in range(int((frame >= 0).sum())):   # filled slots come first; the others hold frame -1
            x0, y0, w, h, s = (float(v) for v in meta[i, 2:7])
            faces[int(frame[i])].append({"box": [x0, y0, x0 + w, y0 + h], "score": s, "row": int(row[i]), "slot": i,
                                         "ident": int(ident[i]), "ident_score": float(score[i])})
        return faces


class PersonRecognition:
    """Who is standing how: ``TopDownPose`` and ``FaceCrops`` on one frame trunk, then
    prpe_face_person_match. ``pose`` / ``faces``: keyword arguments of the two stages (dicts).
    ``kp_thr``, ``head_kpts``: the head point of a skeleton is the mean of its first ``head_kpts``
    keypoints (COCO: nose, eyes, ears) with score >= ``kp_thr``. At most 32 persons and 32 faces
    per frame.
    ``align=True``: the match runs before the crops are made, and the crop of a
    face whose person has both eyes and the nose at or above ``kp_thr`` is registered on the ArcFace
    template the face branch was trained with (prpe_face_align_fit, prpe_roi_warp); every other face
    keeps its window. ``align_scale`` = (lo, hi) bounds the aligned crop's width over the window's.
    ``person_face`` does not depend on it; the output gains ``"face_warp"``. Enrol through
    ``PersonRecognition.enrol`` then, so that gallery rows and probes share a geometry."""

    def __init__(self, model, gallery, pose=None, faces=None, kp_thr=0.3, head_kpts=arch.HEAD_KEYPOINTS, align=False,
                 align_scale=(0.5, 2.0)):
        self.pose = TopDownPose(model, **dict(pose or {}))
        self.faces = FaceCrops(model, gallery, **dict(faces or {}))
        if self.pose.branch != "yolo_person":
            raise ValueError("PersonRecognition: the pose stage runs on the person head")
        for name, stage in (("pose", self.pose), ("faces", self.faces)):
            if stage.max_per_frame > ops.MATCH_MAX_PER_FRAME:
                raise ValueError(f"PersonRecognition: {name} max_per_frame = {stage.max_per_frame}; the match takes "
                                 f"at most {ops.MATCH_MAX_PER_FRAME} per frame")
        if not 1 <= int(head_kpts) <= arch.NUM_KEYPOINTS or float(kp_thr) != float(kp_thr):
            raise ValueError(f"PersonRecognition: head_kpts must be in 1..{arch.NUM_KEYPOINTS} and kp_thr a number")
        lo, hi = (float(v) for v in align_scale)
        if not 0.0 < lo <= hi:
            raise ValueError(f"PersonRecognition: align_scale = {(lo, hi)} must satisfy 0 < lo <= hi")
        self.model, self.kp_thr, self.head_kpts = model, float(kp_thr), int(head_kpts)
        self.align, self.align_scale = bool(align), (lo, hi)

    def _detect(self, feat):
        """Both heads on the frame features: before any crop's trunk call re-zeroes the trunk's
        max|x| pool (Engine.feat_prec)."""
        m = self.model
        e = m.engine
        pd = non_max_suppression_padded(e.yolo("yolo_person", feat, m._stride(m.yolo_person)))
        fd = non_max_suppression_padded(e.yolo("yolo_face", feat, m._stride(m.yolo_face)))
        return pd, fd

    def _detect_u8(self, frames_u8, ingest):
        """``_detect`` on uint8 source frames, both detectors' boxes back in SOURCE pixels."""
        (pd, pc), (fd, fc) = self._detect(self.model.engine.trunk_u8(frames_u8, ingest))
        src = frames_u8.shape[1:3]
        pd = _to_source(pd, _scale_xy(self.pose.box_scale, ingest.size), ingest, src)
        fd = _to_source(fd, _scale_xy(self.faces.box_scale, ingest.size), ingest, src)
        return (pd, pc), (fd, fc)

    # ------------------------------------------------------------------ entry points
    @torch.no_grad()
    def __call__(self, frames):
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        (pd, pc), (fd, fc) = self._detect(m.engine.trunk(x))
        return self.from_detections(x, pd, pc, fd, fc)

    @torch.no_grad()
    def from_detections(self, frames, person_dets, person_counts, face_dets, face_counts):
        """Enter after NMS with both detectors' padded outputs (``TopDownPose.from_detections`` and
        ``FaceCrops.from_detections`` say what they hold)."""
        return self.from_pose(frames, self.pose.from_detections(frames, person_dets, person_counts), face_dets,
                              face_counts)

    @torch.no_grad()
    def from_pose(self, frames, out_p, face_dets, face_counts):
        """Enter after the pose stage: ``out_p`` is a ``TopDownPose`` output dict for ``frames``
        (its keypoints may come from elsewhere), the faces as ``FaceCrops.from_detections``."""
        if not self.align:
            return self._match(out_p, self.faces.from_detections(frames, face_dets, face_counts), frames.shape[0])
        return self._join(out_p, *self._aligned(frames, out_p, face_dets, face_counts))

    @torch.no_grad()
    def from_frames_u8(self, frames_u8, ingest=None):
        """uint8 source frames [B, Hs, Ws, 3]: one ``trunk_u8``, both heads, then both stages from
        the source frames; boxes, keypoints and windows in SOURCE pixels."""
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest)
        m._sync_weights()
        (pd, pc), (fd, fc) = self._detect_u8(frames_u8, ingest)
        return self.from_pose_u8(frames_u8, self.pose.from_detections_u8(frames_u8, pd, pc, ingest), fd, fc, ingest)

    @torch.no_grad()
    def from_pose_u8(self, frames_u8, out_p, face_dets, face_counts, ingest=None):
        """``from_pose`` with uint8 source frames: ``out_p`` and ``face_dets`` in SOURCE pixels."""
        if not self.align:
            out_f = self.faces.from_detections_u8(frames_u8, face_dets, face_counts, ingest)
            return self._match(out_p, out_f, frames_u8.shape[0])
        return self._join(out_p, *self._aligned_u8(frames_u8, out_p, face_dets, face_counts, ingest))

    # ------------------------------------------------------------------ the match and the aligned face stage
    def _match_lists(self, out_p, meta_f, n_f, ident, score, B):
        P = out_p["crop_meta"].shape[0]
        dev = out_p["crop_meta"].device
        face = torch.empty(P, device=dev, dtype=torch.int32)
        p_ident = torch.empty(P, device=dev, dtype=torch.int64)
        p_score = torch.empty(P, device=dev, dtype=torch.float32)
        status = torch.empty(B, device=dev, dtype=torch.int32)
        ops.face_person_match(out_p["crop_meta"], out_p["n_crops"], out_p["keypoints"], meta_f, n_f, ident, score, B,
                              face_slot=face, person_ident=p_ident, person_score=p_score, status=status,
                              kp_thr=self.kp_thr, head_kpts=self.head_kpts)
        return {"person_face": face, "person_ident": p_ident, "person_score": p_score, "match_status": status}

    def _match(self, out_p, out_f, B):
        return {"pose": out_p, "faces": out_f,
                **self._match_lists(out_p, out_f["crop_meta"], out_f["n_crops"], out_f["ident"], out_f["score"], B)}

    def _rows(self, out_p, B, held):
        """The ``warp`` callback of ``FaceCrops._crops_to_identities``: the match on the finished
        face list with nobody identified yet (the pairing does not look at identities), kept in
        ``held``, then the fit."""
        def rows(meta, n_crops):
            F = meta.shape[0]
            ident = torch.full((F,), -1, device=meta.device, dtype=torch.int64)
            score = torch.full((F,), float("-inf"), device=meta.device, dtype=torch.float32)
            held.update(self._match_lists(out_p, meta, n_crops, ident, score, B))
            warp = torch.zeros(F, ops.WARP_COLS, device=meta.device, dtype=torch.float32)
            return ops.face_align_fit(meta, n_crops, out_p["n_crops"], out_p["keypoints"], held["person_face"],
                                      arch.FACE_IMG, warp=warp, kp_thr=self.kp_thr, scale=self.align_scale)
        return rows

    def _aligned(self, frames, out_p, dets, counts, **kw):
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        B, _, H, W = x.shape
        held = {}
        out_f = self.faces._crops_to_identities(
            B, (H, W), dets, counts, _scale_xy(self.faces.box_scale, (H, W)),
            lambda meta, n_crops, y, amax, warp: ops.roi_warp(x, meta, n_crops, warp, y, y_amax=amax),
            warp=self._rows(out_p, B, held), **kw)
        return out_f, held

    def _aligned_u8(self, frames_u8, out_p, dets, counts, ingest, **kw):
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest)
        m._sync_weights()
        B, Hs, Ws = frames_u8.shape[:3]
        held = {}
        out_f = self.faces._crops_to_identities(
            B, (Hs, Ws), dets, counts, (1.0, 1.0),
            lambda meta, n_crops, y, amax, warp: nv12.roi_warp_src(frames_u8, meta, n_crops, warp, y, ingest,
                                                                  y_amax=amax),
            warp=self._rows(out_p, B, held), **kw)
        return out_f, held

    @staticmethod
    def _join(out_p, out_f, held):
        """Identities to the persons the match paired before the crops were made (on the device)."""
        face = held["person_face"]
        hit = face >= 0
        at = face.clamp(min=0).long()
        ident = torch.where(hit, out_f["ident"][at], torch.full_like(held["person_ident"], -1))
        score = torch.where(hit, out_f["score"][at], torch.full_like(held["person_score"], float("-inf")))
        out_f = dict(out_f)
        warp = out_f.pop("warp")
        return {"pose": out_p, "faces": out_f, "person_face": face, "person_ident": ident, "person_score": score,
                "match_status": held["match_status"], "face_warp": warp}

    # ------------------------------------------------------------------ enrolment (one host read)
    @torch.no_grad()
    def enrol(self, frames, labels):
        """``FaceCrops.enrol`` with the crop this instance's probes get: the best face of every
        frame, aligned to its person's eyes and nose when ``align`` and the gates allow it. Returns
        the indices of the frames that contributed no face."""
        if not self.align:
            return self.faces.enrol(frames, labels)
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        (pd, pc), (fd, fc) = self._detect(m.engine.trunk(x))
        return self.enrol_pose(x, self.pose.from_detections(x, pd, pc), fd, fc, labels)

    @torch.no_grad()
    def enrol_pose(self, frames, out_p, face_dets, face_counts, labels):
        """``enrol`` entered after the pose stage (``from_pose``'s arguments)."""
        if not self.align:
            return self.faces.enrol_detections(frames, face_dets, face_counts, labels)
        out_f, _ = self._aligned(frames, out_p, face_dets, face_counts, max_per_frame=1, identify=False)
        return self.faces._enrol(out_f, labels, frames.shape[0])

    @torch.no_grad()
    def enrol_u8(self, frames_u8, labels, ingest=None):
        """``enrol`` on uint8 source frames [B, Hs, Ws, 3] (``from_frames_u8``)."""
        if not self.align:
            return self.faces.enrol_u8(frames_u8, labels, ingest)
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest)
        m._sync_weights()
        (pd, pc), (fd, fc) = self._detect_u8(frames_u8, ingest)
        out_p = self.pose.from_detections_u8(frames_u8, pd, pc, ingest)
        out_f, _ = self._aligned_u8(frames_u8, out_p, fd, fc, ingest, max_per_frame=1, identify=False)
        return self.faces._enrol(out_f, labels, frames_u8.shape[0])

    @staticmethod
    def results(out):
        """Host view of one call's output (one device-to-host read): per frame, a list of
        ``{"box", "score", "keypoints" [17, 3], "row"`` (as ``TopDownPose.results``), ``"ident"``
        (-1: nobody), ``"ident_score"`` (-inf without a face), ``"face_box"`` ([x0, y0, x1, y1] of
        the matched face's window, or None), ``"face_aligned"`` (the matched face's crop was
        registered to this skeleton's eyes and nose)``}`` in detection order."""
        p, f = out["pose"], out["faces"]
        cols, K = ops.CROP_META_COLS, arch.NUM_KEYPOINTS
        P, F = p["crop_meta"].shape[0], f["crop_meta"].shape[0]
        parts = [p["crop_meta"], p["keypoints"], out["person_score"], f["crop_meta"]]
        flags = [out["face_warp"][:, 0].contiguous().view(torch.int32)] if "face_warp" in out else []
        flat = torch.cat([t.reshape(-1).view(torch.int32) for t in parts] +
                         [out["person_face"], out["person_ident"].view(torch.int32)] + flags).cpu()      # the one read
        sizes = [P * cols, P * K * 3, P, F * cols, P, 2 * P] + [F] * len(flags)
        pm, kp, sc, fm, face, ident, *flags = torch.split(flat, sizes)
        pmi = pm.view(P, cols)
        pm, fm = pmi.view(torch.float32), fm.view(torch.float32).view(F, cols)
        kp, sc = kp.view(torch.float32).view(P, K, 3), sc.view(torch.float32)
        ident = ident.clone().view(torch.int64)    # a copy: an int64 view needs an aligned start
        people = [[] for _ in range(p["counts"].shape[0])]
        for i in range(int((pmi[:, 0] >= 0).sum())):
            x0, y0, w, h, s = (float(v) for v in pm[i, 2:7])
            fs = int(face[i])
            fb = None
            if fs >= 0:
                fx, fy, fw, fh = (float(v) for v in fm[fs, 2:6])
                fb = [fx, fy, fx + fw, fy + fh]
            people[int(pmi[i, 0])].append({"box": [x0, y0, x0 + w, y0 + h], "score": s, "keypoints": kp[i],
                                           "row": int(pmi[i, 1]), "ident": int(ident[i]),
                                           "ident_score": float(sc[i]), "face_box": fb,
                                           "face_aligned": bool(fs >= 0 and flags and int(flags[0][fs]) == 1)})
        return people
