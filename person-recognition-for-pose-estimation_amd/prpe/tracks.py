"""Persons tracked across frames on the device (csrc/track.hip behind
prpe_track_update).

    people = PersonRecognition(model, gallery)
    tracker = PersonTracker(people, n_streams=4)          # four cameras
    out = tracker(frames)                                  # [B,3,H,W], frame b is camera b % 4; no host read
    persons = tracker.results(out)                         # per frame: box, keypoints, ident, track_id, ...
    Annotator(colour_by="track")(frames_u8, out, coords_hw=frames.shape[2:])   # drawn on the device (prpe.annotate)

``PersonRecognition`` answers "who is standing how" for one frame; the tracker says that skeleton 3
of this frame is skeleton 1 of the previous one, and keeps the name a face once gave a track over
the frames in which the face is hidden. The state (32 track slots per stream) lives in device
tensors this object owns and persists between calls; one call is one launch of one wavefront per
stream, which walks the stream's frames of the batch in order.

    tracker = PersonTracker(people, n_streams=4, templates="norm")   # track-level face templates (§5o)
    out = tracker(frames)                                  # + template_ident, template_score, template_faces

With ``templates`` the embeddings of a track's faces are summed into one template per track
(csrc/tracktemplate.hip), and the gallery is asked about the template: many frames that each stay
under the threshold add up to a name, and one false accept among many frames does not keep it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .evalsteps import COCO_SIGMAS
from .faces import PersonRecognition

DEFAULT_GATE = {"iou": 0.7, "pose": 1.0}


def coco_k2(sigmas=COCO_SIGMAS):
    """k2[k] = (2 sigma_k)^2 in fp32: the per-keypoint constant of the pose cost."""
    two = np.float32(2.0) * np.asarray(sigmas, dtype=np.float32)
    return [float(v) for v in two * two]


class PersonTracker:
    """``recognition``: a PersonRecognition. ``n_streams``: independent streams (cameras), each
    with its own 32 track slots and its own ids from 0. ``mode``: "iou" associates on 1 - IoU of
    the person windows, "pose" on the mean over the common keypoints (score >= ``kp_thr`` on both
    sides, at least ``min_common`` of them) of squared distance / (window area * (2 sigma_k)^2).
    ``gate``: the largest cost a match may have (default 0.7 for "iou", 1.0 for "pose").
    ``new_thr``: the detection score an unmatched person needs to open a track. ``max_age``: the
    number of consecutive frames a track may go unmatched before its slot is freed.

    ``frame_stream`` ([B] int32 device tensor, or a sequence) names the stream of every frame of a
    call; a value outside [0, n_streams) leaves the frame untracked. The default is
    ``arange(B) % n_streams``: interleaved cameras, time-major (frames 0 .. n_streams - 1 are the
    cameras' first frames, the next n_streams their second, ...). A stream's frames are taken in
    ascending order, and the frames of one call follow those of the call before.

    ``templates``: None (the default: no template, no further launch, no further key), "norm" or
    "uniform". Otherwise every face matched to a tracked person is added to its track's template,
    weighted by its feature norm (AdaFace's quality signal) or by 1, faces with a norm below
    ``min_norm`` left out; the templates that changed are identified against the recognition stage's
    gallery at its threshold, and ``update`` also returns ``template_ident``, ``template_score`` and
    ``template_faces`` per person. ``track_ident`` stays the best single frame's name. To colour an
    ``Annotator``'s drawing by template, hand it ``{**out, "track_ident": out["template_ident"]}``."""

    def __init__(self, recognition, n_streams=1, mode="iou", gate=None, kp_thr=0.3, min_common=3, new_thr=0.5,
                 max_age=30, k2=None, templates=None, min_norm=0.0):
        if not isinstance(recognition, PersonRecognition):
            raise ValueError(f"PersonTracker: recognition must be a prpe.PersonRecognition, got "
                             f"{type(recognition).__name__}")
        if mode not in ops.TRACK_MODES:
            raise ValueError(f"PersonTracker: mode must be one of {sorted(ops.TRACK_MODES)}, got {mode!r}")
        gate = DEFAULT_GATE[mode] if gate is None else float(gate)
        self.k2 = coco_k2() if k2 is None else [float(v) for v in k2]
        K = len(self.k2)
        if int(n_streams) < 1:
            raise ValueError(f"PersonTracker: n_streams must be at least 1, got {n_streams}")
        if gate != gate or float(kp_thr) != float(kp_thr) or float(new_thr) != float(new_thr):
            raise ValueError("PersonTracker: gate, kp_thr and new_thr must be numbers")
        if not 1 <= int(min_common) <= K or int(max_age) < 0:
            raise ValueError(f"PersonTracker: min_common must be in 1..{K} and max_age at least 0")
        if not 1 <= K <= ops.TRACK_MAX_K or not all(0.0 < v < float("inf") for v in self.k2):
            raise ValueError(f"PersonTracker: k2 must hold 1..{ops.TRACK_MAX_K} finite positive values")
        self.recognition, self.n_streams, self.mode, self.gate = recognition, int(n_streams), mode, gate
        self.kp_thr, self.min_common, self.new_thr, self.max_age = float(kp_thr), int(min_common), float(new_thr), int(max_age)
        if templates is not None and templates not in ops.TEMPLATE_WEIGHTS:
            raise ValueError(f"PersonTracker: templates must be None or one of {sorted(ops.TEMPLATE_WEIGHTS)}, got "
                             f"{templates!r}")
        if float(min_norm) != float(min_norm):
            raise ValueError("PersonTracker: min_norm must be a number")
        self.templates, self.min_norm = templates, float(min_norm)
        self.state = None
        self.template_state = None

    # ------------------------------------------------------------------ state
    def _state(self, dev):
        if self.state is None or self.state["trk_meta"].device != dev:
            S, T, K = self.n_streams, ops.TRACK_SLOTS, len(self.k2)
            self.state = {"trk_meta": torch.zeros(S, T, 8, device=dev, dtype=torch.float32),
                          "trk_kpts": torch.zeros(S, T, K, 3, device=dev, dtype=torch.float32),
                          "trk_ident": torch.empty(S, T, device=dev, dtype=torch.int64),
                          "trk_iscore": torch.empty(S, T, device=dev, dtype=torch.float32),
                          "next_id": torch.empty(S, device=dev, dtype=torch.int32)}
            self.template_state = None
            self.reset()
        return self.state

    def _template_state(self, dev, D):
        """The templates' state, beside the tracker's own: made with the first update, for the
        embedding width it sees. It lives and dies with the tracker's state: an update on another
        device starts tracks and templates afresh (``_state``). An update whose embeddings have
        another width while templates exist is refused, since it would forget every template but
        keep the tracks; ``reset()`` does not change the width."""
        ts = self.template_state
        if ts is not None and ts["tmpl_sum"].device == dev and ts["tmpl_sum"].shape[2] != D:
            raise ValueError(f"PersonTracker: the templates sum {ts['tmpl_sum'].shape[2]}-d embeddings, this update brings "
                             f"{D}-d ones")
        if ts is None or ts["tmpl_sum"].device != dev:
            S, T = self.n_streams, ops.TRACK_SLOTS
            self.template_state = {"tmpl_owner": torch.full((S, T), -1, device=dev, dtype=torch.int32),
                                   "tmpl_sum": torch.zeros(S, T, D, device=dev, dtype=torch.int64),
                                   "tmpl_n": torch.zeros(S, T, device=dev, dtype=torch.int32),
                                   "tmpl_ident": torch.full((S, T), -1, device=dev, dtype=torch.int64),
                                   "tmpl_score": torch.full((S, T), float("-inf"), device=dev, dtype=torch.float32)}
        return self.template_state

    def reset(self, streams=None):
        """Forget every track of ``streams`` (a sequence of stream indices; default: all) and
        start their ids from 0 again, their templates with them. Plain fills on the device."""
        st = self.state
        if st is None:
            return
        sel = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.int64,
                                                                  device=st["next_id"].device)
        ts = self.template_state
        if ts is not None:
            ts["tmpl_owner"][sel] = -1
            ts["tmpl_sum"][sel] = 0
            ts["tmpl_n"][sel] = 0
            ts["tmpl_ident"][sel] = -1
            ts["tmpl_score"][sel] = float("-inf")
        st["trk_meta"].view(torch.int32)[sel] = 0
        st["trk_meta"].view(torch.int32)[sel, :, 0] = -1
        st["trk_kpts"][sel] = 0.0
        st["trk_ident"][sel] = -1
        st["trk_iscore"][sel] = float("-inf")
        st["next_id"][sel] = 0

    # ------------------------------------------------------------------ entry points
    @torch.no_grad()
    def __call__(self, frames, frame_stream=None):
        return self.update(self.recognition(frames), frame_stream)

    @torch.no_grad()
    def from_frames_u8(self, frames_u8, ingest=None, frame_stream=None):
        return self.update(self.recognition.from_frames_u8(frames_u8, ingest), frame_stream)

    @torch.no_grad()
    def update(self, out, frame_stream=None):
        """One prpe_track_update on a ``PersonRecognition`` output: returns ``out`` extended by
        ``track_id``, ``track_hits`` [P] int32, ``track_ident`` [P] int64, ``track_ident_score``
        [P] and ``track_status`` [B] int32. With ``templates``: then prpe_track_template_update, the
        gallery search on the templates that changed and prpe_track_template_assign, and also
        ``template_ident`` [P] int64, ``template_score`` [P] and ``template_faces`` [P] int32 (the
        name, the score and the number of faces of the person's track's template; -1, -inf, 0
        without a track). The state advances; nothing is read from the device."""
        p = out["pose"]
        meta = p["crop_meta"]
        dev, P, B = meta.device, meta.shape[0], p["counts"].shape[0]
        if frame_stream is None:
            fs = torch.arange(B, device=dev, dtype=torch.int32) % self.n_streams
        elif isinstance(frame_stream, torch.Tensor):
            fs = frame_stream.to(device=dev, dtype=torch.int32).contiguous()
        else:
            fs = torch.tensor([int(v) for v in frame_stream], dtype=torch.int32).to(dev)
        if fs.shape != (B,):
            raise ValueError(f"PersonTracker: frame_stream must name the stream of each of the {B} frames")
        st = self._state(dev)
        tid = torch.empty(P, device=dev, dtype=torch.int32)
        hits = torch.empty(P, device=dev, dtype=torch.int32)
        ident = torch.empty(P, device=dev, dtype=torch.int64)
        iscore = torch.empty(P, device=dev, dtype=torch.float32)
        status = torch.empty(B, device=dev, dtype=torch.int32)
        ops.track_update(meta, p["n_crops"], p["keypoints"], out["person_ident"], out["person_score"], fs,
                         track_id=tid, track_hits=hits, track_ident=ident, track_iscore=iscore, status=status,
                         k2=self.k2, mode=self.mode, gate=self.gate, kp_thr=self.kp_thr, min_common=self.min_common,
                         new_thr=self.new_thr, max_age=self.max_age, **st)
        res = {**out, "track_id": tid, "track_hits": hits, "track_ident": ident, "track_ident_score": iscore,
               "track_status": status}
        if self.templates is not None:
            res.update(self._templates(out, fs, tid))
        return res

    def _templates(self, out, fs, tid):
        p, f = out["pose"], out["faces"]
        meta, emb = p["crop_meta"], f["embeddings"]
        dev, P, (F, D) = meta.device, meta.shape[0], emb.shape
        S, T = self.n_streams, ops.TRACK_SLOTS
        ts = self._template_state(dev, D)
        Q = min(S * T, F)
        rows = torch.empty(Q, device=dev, dtype=torch.int32)
        n_dirty = torch.empty(1, device=dev, dtype=torch.int32)
        pos = torch.empty(S, T, device=dev, dtype=torch.int32)
        queries = torch.empty(Q, D, device=dev, dtype=torch.float32)
        trk_meta = self.state["trk_meta"]
        ops.track_template_update(meta, p["n_crops"], tid, out["person_face"], emb, f["norms"], f["n_crops"], fs, trk_meta,
                                  dirty_rows=rows, n_dirty=n_dirty, dirty_pos=pos, queries=queries,
                                  weight=self.templates, min_norm=self.min_norm, **ts)
        faces = self.recognition.faces
        if faces.gallery is not None and len(faces.gallery) > 0:
            q_ident, q_score = faces.gallery.identify(queries, faces.threshold)
        else:                                            # nobody is enrolled: every template stays unnamed
            q_ident = torch.full((Q,), -1, device=dev, dtype=torch.int64)
            q_score = torch.full((Q,), float("-inf"), device=dev, dtype=torch.float32)
        t_ident = torch.empty(P, device=dev, dtype=torch.int64)
        t_score = torch.empty(P, device=dev, dtype=torch.float32)
        t_faces = torch.empty(P, device=dev, dtype=torch.int32)
        ops.track_template_assign(meta, p["n_crops"], tid, fs, trk_meta, q_ident, q_score, n_dirty, rows, pos,
                                  tmpl_n=ts["tmpl_n"], tmpl_ident=ts["tmpl_ident"], tmpl_score=ts["tmpl_score"],
                                  template_ident=t_ident, template_score=t_score, template_faces=t_faces)
        return {"template_ident": t_ident, "template_score": t_score, "template_faces": t_faces}

    # ------------------------------------------------------------------ templates on the host (not the live path)
    def _template_rows(self, streams):
        """(track ids, owners, faces, idents, scores) of ``streams``' slots on the host: one read."""
        if self.state is None or self.template_state is None:
            return None
        ts, sel = self.template_state, torch.as_tensor(list(streams), dtype=torch.int64, device=self.state["next_id"].device)
        ids = self.state["trk_meta"].view(torch.int32)[sel, :, 0]
        parts = [ids, ts["tmpl_owner"][sel], ts["tmpl_n"][sel], ts["tmpl_score"][sel], ts["tmpl_ident"][sel]]
        flat = torch.cat([t.reshape(-1).view(torch.int32) for t in parts]).cpu()          # the one read
        host = []
        for t, piece in zip(parts, torch.split(flat, [t.numel() * t.element_size() // 4 for t in parts])):
            host.append(piece.clone().view(t.dtype).view(t.shape))
        return host

    def templates_host(self):
        """Per stream the templates of its live tracks, in slot order: a list of dicts ``track_id``,
        ``faces``, ``ident`` and ``score``. One device-to-host read; not the live path."""
        host = self._template_rows(range(self.n_streams))
        if host is None:
            return [[] for _ in range(self.n_streams)]
        ids, owner, n, score, ident = host
        return [[{"track_id": int(ids[s, j]), "faces": int(n[s, j]), "ident": int(ident[s, j]), "score": float(score[s, j])}
                 for j in range(ids.shape[1]) if int(ids[s, j]) >= 0 and int(owner[s, j]) == int(ids[s, j])]
                for s in range(self.n_streams)]

    def enrol_track(self, stream, track_id, label):
        """Append the fused template of track ``track_id`` of ``stream`` to the recognition stage's
        gallery as ``label`` (``FaceGallery.add`` normalises it). Raises for a track that is not live
        or has no faces. One device-to-host read, as ``FaceCrops.enrol`` has; returns the gallery
        rows (first, last + 1)."""
        stream, track_id = int(stream), int(track_id)
        gallery = self.recognition.faces.gallery
        if gallery is None:
            raise ValueError("PersonTracker.enrol_track: no gallery to enrol into")
        if self.templates is None or not 0 <= stream < self.n_streams or track_id < 0:
            raise ValueError(f"PersonTracker.enrol_track: no template of track {track_id} of stream {stream}")
        host = self._template_rows([stream])
        slot = [] if host is None else [j for j in range(host[0].shape[1])
                                        if int(host[0][0, j]) == track_id == int(host[1][0, j]) and int(host[2][0, j]) > 0]
        if not slot:
            raise ValueError(f"PersonTracker.enrol_track: track {track_id} of stream {stream} is not live or has no faces")
        row = (self.template_state["tmpl_sum"][stream, slot[0]].to(torch.float64) * 2.0 ** -ops.TEMPLATE_SCALE_BITS)
        return gallery.add(row.to(torch.float32)[None], [int(label)])

    @staticmethod
    def results(out):
        """``PersonRecognition.results`` with ``"track_id"`` (-1: no track), ``"track_hits"``,
        ``"track_ident"`` (the track's name: -1 until a face gave one) and ``"track_ident_score"``
        per person, and ``"template_ident"``, ``"template_score"`` and ``"template_faces"`` when the
        tracker keeps templates. One device-to-host read for everything."""
        p, f = out["pose"], out["faces"]
        parts = [p["crop_meta"], p["keypoints"], out["person_score"], f["crop_meta"], out["person_face"],
                 out["person_ident"], out["track_id"], out["track_hits"], out["track_ident_score"], out["track_ident"]]
        fused = "template_ident" in out
        if fused:
            parts += [out["template_faces"], out["template_score"], out["template_ident"]]
        flat = torch.cat([t.reshape(-1).view(torch.int32) for t in parts]).cpu()          # the one read
        host = []
        for t, piece in zip(parts, torch.split(flat, [t.numel() * t.element_size() // 4 for t in parts])):
            host.append(piece.clone().view(t.dtype).view(t.shape))       # a copy: an int64 view needs an aligned start
        pm, kp, sc, fm, face, ident, tid, hits, tsc, tident = host[:10]
        people = PersonRecognition.results({"pose": {**p, "crop_meta": pm, "keypoints": kp},
                                            "faces": {**f, "crop_meta": fm}, "person_face": face,
                                            "person_ident": ident, "person_score": sc})
        frame = pm.view(torch.int32)[:, 0]
        seen = [0] * len(people)
        for i in range(int((frame >= 0).sum())):     # the slots in the order PersonRecognition.results lists them
            b = int(frame[i])
            people[b][seen[b]].update({"track_id": int(tid[i]), "track_hits": int(hits[i]),
                                       "track_ident": int(tident[i]), "track_ident_score": float(tsc[i])})
            if fused:
                people[b][seen[b]].update({"template_ident": int(host[12][i]), "template_score": float(host[11][i]),
                                           "template_faces": int(host[10][i])})
            seen[b] += 1
        return people
