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
    ascending order, and the frames of one call follow those of the call before."""

    def __init__(self, recognition, n_streams=1, mode="iou", gate=None, kp_thr=0.3, min_common=3, new_thr=0.5,
                 max_age=30, k2=None):
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
        self.state = None

    # ------------------------------------------------------------------ state
    def _state(self, dev):
        if self.state is None or self.state["trk_meta"].device != dev:
            S, T, K = self.n_streams, ops.TRACK_SLOTS, len(self.k2)
            self.state = {"trk_meta": torch.zeros(S, T, 8, device=dev, dtype=torch.float32),
                          "trk_kpts": torch.zeros(S, T, K, 3, device=dev, dtype=torch.float32),
                          "trk_ident": torch.empty(S, T, device=dev, dtype=torch.int64),
                          "trk_iscore": torch.empty(S, T, device=dev, dtype=torch.float32),
                          "next_id": torch.empty(S, device=dev, dtype=torch.int32)}
            self.reset()
        return self.state

    def reset(self, streams=None):
        """Forget every track of ``streams`` (a sequence of stream indices; default: all) and
        start their ids from 0 again. Plain fills on the device."""
        st = self.state
        if st is None:
            return
        sel = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.int64,
                                                                  device=st["next_id"].device)
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
        [P] and ``track_status`` [B] int32. The state advances; nothing is read from the device."""
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
        return {**out, "track_id": tid, "track_hits": hits, "track_ident": ident, "track_ident_score": iscore,
                "track_status": status}

    @staticmethod
    def results(out):
        """``PersonRecognition.results`` with ``"track_id"`` (-1: no track), ``"track_hits"``,
        ``"track_ident"`` (the track's name: -1 until a face gave one) and ``"track_ident_score"``
        per person. One device-to-host read for everything."""
        p, f = out["pose"], out["faces"]
        parts = [p["crop_meta"], p["keypoints"], out["person_score"], f["crop_meta"], out["person_face"],
                 out["person_ident"], out["track_id"], out["track_hits"], out["track_ident_score"], out["track_ident"]]
        flat = torch.cat([t.reshape(-1).view(torch.int32) for t in parts]).cpu()          # the one read
        host = []
        for t, piece in zip(parts, torch.split(flat, [t.numel() * t.element_size() // 4 for t in parts])):
            host.append(piece.clone().view(t.dtype).view(t.shape))       # a copy: an int64 view needs an aligned start
        pm, kp, sc, fm, face, ident, tid, hits, tsc, tident = host
        people = PersonRecognition.results({"pose": {**p, "crop_meta": pm, "keypoints": kp},
                                            "faces": {**f, "crop_meta": fm}, "person_face": face,
                                            "person_ident": ident, "person_score": sc})
        frame = pm.view(torch.int32)[:, 0]
        seen = [0] * len(people)
        for i in range(int((frame >= 0).sum())):     # the slots in the order PersonRecognition.results lists them
            b = int(frame[i])
            people[b][seen[b]].update({"track_id": int(tid[i]), "track_hits": int(hits[i]),
                                       "track_ident": int(tident[i]), "track_ident_score": float(tsc[i])})
            seen[b] += 1
        return people
