"""Device halves of the reference eval steps that wrap the model.

* ``pose_flip_test``  — PoseEstimationModule.validation_step's flip test
  (training/lightning/pose_estimation/module.py:466-484): heatmaps of the frames and of the
  W-mirrored frames (the mirror is a negative-stride read in the stem's layout kernel, no
  flipped copy), flipped back and averaged by one kernel (prpe_flip_average). ``mode``:
  "reference" reproduces ``flipped[:, pair] = flipped[:, pair].flip(0)`` literally (that
  reverses the BATCH order of the paired channels); "swap" exchanges the pair's channels.
* ``FaceRecognitionEval`` — FaceRecognitionModule.validation_step's head
  (training/lightning/face_recognition/module.py:133-145): F.normalize of the [512, classes]
  head kernel (rows, dim=1) once per kernel, then per batch F.normalize(embeddings), the
  [B,512] x [512,classes] cosine GEMM with the scale s folded into the epilogue (prpe_conv2d,
  fp32-faithful 3-plane mode), and cross-entropy + argmax + accuracy on device
  (prpe_ce_argmax).
* ``DetectionMetricsDevice`` — the detection validation step's DetectionMetrics
  (training/lightning/face_detection/module_v2.py:13-127, driven by validation_step :458-499):
  per batch one launch matches the padded NMS output against the ground truth and appends
  (score, best IoU) records on device (prpe_det_metrics_update); compute() at epoch end
  (prpe_det_metrics_compute) returns the reference's dict.
* ``detection_eval_loss`` — the same step's compute_loss (module_v2.py:178-303) on the eval
  head output: one block per image (confidence filter, IoU matching, the pairwise CIoU mean,
  cross-entropy, background BCE), no per-image host sync (prpe_det_eval_loss).
* ``PoseEvalStep`` — the rest of PoseEstimationModule.validation_step (module.py:451-570) after
  the two model passes: one launch averages the flip test in registers, rebuilds the target of
  ``_generate_target_heatmap`` per pixel, and gives JointsMSELoss's OHKM loss and the soft-argmax
  (prpe_pose_eval_loss); a second appends the COCO keypoint records on device
  (prpe_pose_coco_records). The host only looks the image ids up in its set; ``predictions()``
  reads the records once per epoch.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .pack import pack_matrix

F_NORMALIZE_EPS = 1e-12          # torch.nn.functional.normalize default eps
COCO_FLIP_PAIRS = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]  # datamodule.py:25-34
# OKS sigmas of the 17 COCO keypoints (datamodule.py:37-40), fp32 as there
COCO_SIGMAS = np.array([.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062,
                        .107, .107, .087, .087, .089, .089], dtype=np.float32)


def flip_partner(k: int = 17, pairs=COCO_FLIP_PAIRS) -> list[int]:
    part = [-1] * k
    for a, b in pairs:
        part[a], part[b] = b, a
    return part


@torch.no_grad()
def pose_flip_test(model, images, mode: str = "reference"):
    """Averaged flip-test heatmaps [B,17,64,48] for ``images`` [B,3,H,W] (module.py:466-484)."""
    if mode not in ("reference", "swap"):
        raise ValueError(f"unknown flip mode {mode!r}")
    x = model._check_input(images)
    model._sync_weights()                         # repack if a weight changed in place
    e = model.engine
    heat = e.vitpose(e.trunk(x))
    heat_f = e.vitpose(e.trunk(x, flip_w=True))
    return ops.flip_average(heat, heat_f, flip_partner(heat.shape[1]), 0 if mode == "reference" else 1)


class FaceRecognitionEval:
    """(loss, acc) of the face-recognition eval step, on device."""

    def __init__(self, model, s: float = 64.0, precision: int = 2):
        kernel = model.ada_face.head.kernel
        if kernel is None:
            raise ValueError("model.ada_face.head.kernel is not set (load a state_dict that has it)")
        self.model = model
        self.s = float(s)
        self.precision = precision
        self.set_kernel(kernel)

    def set_kernel(self, kernel):
        """Normalise + pack the [512, classes] head kernel. An in-place change of ``kernel``
        (the model's ``ada_face.head.kernel`` parameter) is detected by its version counter at
        the next call and repacked, as ``CombinedModel`` does for its weights."""
        self._kernel, self._kernel_version = kernel, kernel._version
        k = kernel.to(self.model.device, torch.float32).contiguous()
        d, ncls = k.shape
        kn = torch.empty_like(k)
        ops.l2norm(k, kn, torch.empty(d, device=k.device), F_NORMALIZE_EPS)   # F.normalize(kernel), dim=1
        self.classes = ncls
        self.pack = pack_matrix("ada_face.head:logits", kn.t().cpu(), 1, 1, d, 1, 0, self.model.device,
                                scale=torch.full((ncls,), self.s))

    def logits(self, embeddings):
        if self._kernel._version != self._kernel_version:
            self.set_kernel(self._kernel)
        B, d = embeddings.shape
        e = embeddings.contiguous().float()
        en = torch.empty_like(e)
        ops.l2norm(e, en, torch.empty(B, device=e.device), F_NORMALIZE_EPS)   # F.normalize(embeddings)
        out = torch.empty(B, 1, 1, self.classes, device=e.device)
        ops.conv2d(en.view(B, 1, 1, d), self.pack, out, precision=self.precision)
        return out.view(B, self.classes)

    @torch.no_grad()
    def __call__(self, images=None, labels=None, embeddings=None):
        """Returns (loss, acc, argmax) as device tensors; pass ``embeddings`` to skip the model."""
        if embeddings is None:
            self.model.set_task("face_recognition")
            embeddings, _ = self.model(images)
        out = self.logits(embeddings)
        loss, amax, summary = ops.ce_argmax(out, labels)
        if labels is None:
            return None, None, amax
        return summary[0], summary[1], amax


class DetectionMetricsDevice:
    """DetectionMetrics with its state on the device (same update/compute semantics)."""

    THRESHOLDS = torch.linspace(0.5, 0.95, 10).tolist()     # module_v2.py:92
    KEYS = ("precision", "recall", "f1", "mAP50", "mAP75", "mAP")

    def __init__(self, device="cuda", capacity: int = 1 << 20):
        self.counters = torch.zeros(4, dtype=torch.int64, device=device)   # tp, fp, gt, records
        self.records = torch.empty(capacity, 2, dtype=torch.float32, device=device)

    def reset(self):
        self.counters.zero_()

    def update_batch(self, dets, counts, gt_boxes, gt_batch):
        """dets [B, max_det, 6] + counts [B] (postproc.non_max_suppression_padded); gt_boxes [G, 4]
        xyxy with gt_batch [G] = the reference's targets['boxes'] / targets['batch_idx']."""
        ops.det_metrics_update(dets, counts, gt_boxes, gt_batch, self.counters, self.records)

    def compute(self) -> dict:
        n = int(self.counters[3].item())          # one host read per epoch
        if n > self.records.shape[0]:
            raise RuntimeError(f"DetectionMetricsDevice: {n} records exceed the capacity {self.records.shape[0]}")
        out = ops.det_metrics_compute(self.counters, self.records, n, self.THRESHOLDS).tolist()
        return dict(zip(self.KEYS, out))


@torch.no_grad()
def detection_eval_loss(det, gt_boxes, gt_batch, gt_labels=None):
    """(avg_loss [1], per_image [B, 4] = (loss_b, box, cls, bg)) for the eval-mode detection
    output ``det`` [B, 4+nc, N] (FaceDetectionModule.process_yolo_output's eval split:
    boxes det[:, :4], scores det[:, 4:]) against targets boxes / batch_idx / labels."""
    return ops.det_eval_loss(det[:, :4], det[:, 4:], gt_boxes, gt_batch, gt_labels)


def joints_mse_keypoint_weights(sigmas=COCO_SIGMAS) -> np.ndarray:
    """JointsMSELoss.__init__'s keypoint weights (module.py:57-58): numpy fp32 1 / (sigma + 1e-8),
    divided by its mean (torch's mean of the same fp32 values)."""
    w = torch.from_numpy(1 / (np.asarray(sigmas, dtype=np.float32) + 1e-8))
    return (w / w.mean()).numpy()


def format_coco_records(rec_kpts, rec_meta, slot_image_ids) -> list[dict]:
    """The reference's prediction dicts (module.py:552-559) from record arrays: rec_kpts [n,K,3]
    fp32 (x, y, v), rec_meta [n,8] fp32 whose first two columns hold int32 bits (image slot, n),
    then score, bbox x 4, area; slot_image_ids maps a slot to its image id."""
    kp = np.asarray(rec_kpts, dtype=np.float32)
    meta = np.ascontiguousarray(rec_meta, dtype=np.float32)
    slots = meta[:, :1].copy().view(np.int32)[:, 0]
    preds = []
    for r in range(kp.shape[0]):
        flat = []
        for x, y, v in kp[r].tolist():
            flat.extend([x, y, int(v)])
        m = meta[r].tolist()
        preds.append({"image_id": int(slot_image_ids[slots[r]]), "category_id": 1, "keypoints": flat,
                      "score": m[2], "bbox": m[3:7], "area": m[7]})
    return preds


# COCOeval's Params for iouType 'keypoints' (fp64, as pycocotools builds them)
COCO_KP_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_KP_AREA_RNGS = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]     # all, medium, large
COCO_KP_STAT_KEYS = ("val/AP", "val/AP50", "val/AP75", "val/APm", "val/APl",
                     "val/AR", "val/AR50", "val/AR75", "val/ARm", "val/ARl")       # module.py:612-622


class CocoKeypointGT:
    """The person keypoint annotations of a COCO file as the table ``prpe_coco_kp_match`` reads:
    images in ascending image-id order (COCOeval's ``params.imgIds``), each image's annotations in
    file order, CSR. Built on the host from plain JSON (no pycocotools); ``to(device)`` uploads
    it once per dataset."""

    MAX_GT = ops.COCO_MAX_GT

    def __init__(self, image_ids, gt_start, kpts, bbox, area, iscrowd, ignore):
        self.image_ids = [int(i) for i in image_ids]
        self.row_of = {i: r for r, i in enumerate(self.image_ids)}
        self.gt_start = np.ascontiguousarray(gt_start, dtype=np.int32)
        self.kpts = np.ascontiguousarray(kpts, dtype=np.float64)
        self.bbox = np.ascontiguousarray(bbox, dtype=np.float64).reshape(-1, 4)
        self.area = np.ascontiguousarray(area, dtype=np.float64)
        self.iscrowd = np.ascontiguousarray(iscrowd, dtype=np.uint8)
        self.ignore = np.ascontiguousarray(ignore, dtype=np.uint8)
        self.K = int(self.kpts.shape[1])
        counts = np.diff(self.gt_start)
        self.max_gt = int(counts.max()) if len(counts) else 0
        if len(self.image_ids) < 1:
            raise ValueError("CocoKeypointGT: no images")
        if self.max_gt > self.MAX_GT:
            worst = self.image_ids[int(counts.argmax())]
            raise ValueError(f"CocoKeypointGT: image {worst} has {self.max_gt} annotations, the device table "
                             f"takes at most {self.MAX_GT} per image")
        self.device = None
        self._dev = None

    @classmethod
    def from_annotations(cls, annotations, image_ids=None, category_id: int = 1, num_keypoints: int | None = None,
                         device=None):
        """``annotations``: a path to a COCO JSON file, its dict ({"images": ..., "annotations": ...})
        or a list of annotation dicts. ``image_ids`` adds images that have no annotation (a dict's
        "images" are added by themselves). Annotations of other categories are left out."""
        if isinstance(annotations, (str, bytes)) or hasattr(annotations, "__fspath__"):
            import json
            with open(annotations) as f:
                annotations = json.load(f)
        ids = set() if image_ids is None else {int(i) for i in image_ids}
        if isinstance(annotations, dict):
            ids |= {int(im["id"]) for im in annotations.get("images", [])}
            annotations = annotations.get("annotations", [])
        anns = [a for a in annotations if int(a.get("category_id", category_id)) == category_id]
        ids |= {int(a["image_id"]) for a in anns}
        ids = sorted(ids)
        per = {i: [] for i in ids}
        for a in anns:
            per[int(a["image_id"])].append(a)
        K = num_keypoints
        if K is None:
            K = len(anns[0]["keypoints"]) // 3 if anns else len(COCO_KP_SIGMAS)
        start, kp, bb, ar, cr, ig = [0], [], [], [], [], []
        for i in ids:
            for a in per[i]:
                k = np.asarray(a["keypoints"], dtype=np.float64)
                if k.shape != (K * 3,):
                    raise ValueError(f"CocoKeypointGT: annotation {a.get('id')} has {k.size} keypoint values, not {K * 3}")
                k = k.reshape(K, 3)
                crowd = bool(a.get("iscrowd", 0))
                nk = a["num_keypoints"] if "num_keypoints" in a else int((k[:, 2] > 0).sum())
                kp.append(k)
                bb.append([float(v) for v in a["bbox"]])
                ar.append(float(a["area"]))
                cr.append(crowd)
                ig.append(crowd or nk == 0)           # COCOeval._prepare for 'keypoints'
            start.append(len(kp))
        gt = cls(ids, start, np.stack(kp) if kp else np.zeros((0, K, 3)), np.asarray(bb, dtype=np.float64), ar, cr, ig)
        return gt if device is None else gt.to(device)

    def __len__(self):
        return len(self.image_ids)

    def to(self, device):
        device = torch.device(device)
        if self._dev is None or self.device != device:
            self._dev = {k: torch.from_numpy(getattr(self, k)).to(device)
                         for k in ("gt_start", "kpts", "bbox", "area", "iscrowd", "ignore")}
            self.device = device
        return self

    def tensors(self) -> dict:
        if self._dev is None:
            raise ValueError("CocoKeypointGT: the table is on the host; call .to(device) first")
        return self._dev

    def slot_to_img(self, slot_image_ids) -> np.ndarray:
        """Row in the table of every image slot of an epoch (int32). An image id that the
        annotations do not know is refused, as ``COCO.loadRes`` asserts."""
        rows = np.empty(len(slot_image_ids), dtype=np.int32)
        for s, i in enumerate(slot_image_ids):
            r = self.row_of.get(int(i))
            if r is None:
                raise ValueError(f"CocoKeypointGT: image id {int(i)} of the results is not in the annotations")
            rows[s] = r
        return rows


def coco_keypoint_eval(rec_kpts, rec_meta, counter, n_max, slot_image_ids, gt: CocoKeypointGT,
                       sigmas=None, want_oks=True) -> dict:
    """``prpe_coco_kp_match`` + ``prpe_coco_kp_accumulate`` on device record arrays. Returns the
    device tensors of both (dt_score, dt_bits, dt_rec, npig, oks, precision, recall, stats); reads
    nothing back."""
    dev = rec_kpts.device
    t = gt.to(dev).tensors()
    sigmas = COCO_KP_SIGMAS if sigmas is None else sigmas
    rows = gt.slot_to_img(slot_image_ids)
    s2i = torch.from_numpy(rows).to(dev) if len(rows) else torch.zeros(1, dtype=torch.int32, device=dev)
    ev = ops.coco_kp_match(rec_kpts, rec_meta, counter, n_max, s2i, t["gt_start"], t["kpts"], t["bbox"], t["area"],
                           t["iscrowd"], t["ignore"], gt.max_gt, sigmas, COCO_IOU_THRS, COCO_KP_AREA_RNGS,
                           want_oks=want_oks)
    ev.update(ops.coco_kp_accumulate(ev["dt_score"], ev["dt_bits"], ev["npig"], COCO_REC_THRS))
    return ev


class PoseEvalStep:
    """PoseEstimationModule.validation_step with everything after the model on the device.

    ``step = PoseEvalStep(model); step.reset(); loss = step(batch); ...; step.compute(gt)`` gives
    on_validation_epoch_end's COCO metrics on the device; ``step.predictions()`` the records.
    ``batch`` is the reference's dict (images, keypoints [B,N,K,3], boxes [B,N,4], areas [B,N],
    masks, is_crowd [B,N], image_ids: host values). With the batch's tensors on the device, as
    the trainer delivers them, a step uploads nothing and never waits for the stream: the keep
    flags of the image ids go to the record kernel as launch arguments."""

    def __init__(self, model=None, heatmap_size=(64, 48), sigma: float = 2.0, keypoint_thresh: float = 0.3,
                 ohkm_topk: int = 8, flip_mode: str = "reference", capacity: int = 1 << 16, device=None):
        if flip_mode not in ("reference", "swap"):
            raise ValueError(f"unknown flip mode {flip_mode!r}")
        self.model = model
        self.device = device if device is not None else (model.device if model is not None else "cuda")
        self.heatmap_size = tuple(heatmap_size)
        self.sigma = float(sigma)
        self.keypoint_thresh = float(keypoint_thresh)
        self.ohkm_topk = int(ohkm_topk)
        self.flip_mode = flip_mode
        self.capacity = int(capacity)
        self.kp_weights = joints_mse_keypoint_weights()
        self._state = None                # (counter, rec_kpts, rec_meta), allocated at the first batch
        self.last = None                  # the last batch's device outputs (loss, per_kp, coords, scores)
        self.last_eval = None             # compute()'s device tensors
        self.reset()

    def reset(self):
        """on_validation_epoch_start (module.py:572-576)."""
        self._seen = set()
        self._slot_ids = []               # image id of every frame of the epoch, by slot
        self._max_records = 0             # host bound on the records written (kept frames x N)
        if self._state is not None:
            self._state[0].zero_()

    def keep_flags(self, image_ids, commit: bool = True) -> list[int]:
        """1 where the image id was not seen before in this epoch, nor earlier in the batch
        (module.py:507-513). The only host work of a step. ``commit`` records the ids as seen and
        by slot; ``__call__`` does that only after both launches succeeded."""
        if isinstance(image_ids, torch.Tensor):
            image_ids = image_ids.tolist()
        ids = [int(i) for i in image_ids]
        new, keep = set(), []
        for i in ids:
            keep.append(0 if i in self._seen or i in new else 1)
            new.add(i)
        if commit:
            self._commit(ids, new)
        return keep

    def _commit(self, ids, new):
        self._seen |= new
        self._slot_ids.extend(ids)

    @torch.no_grad()
    def __call__(self, batch, heatmaps=None, heatmaps_flipped=None):
        """val_loss (a device scalar) of one batch; its records are appended on the device.
        ``heatmaps`` (and ``heatmaps_flipped``, the flipped pass' output) skip the model."""
        if heatmaps is None:
            m = self.model
            x = m._check_input(batch["images"])
            m._sync_weights()
            e = m.engine
            heatmaps = e.vitpose(e.trunk(x))
            heatmaps_flipped = e.vitpose(e.trunk(x, flip_w=True))
        B, K, H, W = heatmaps.shape
        if (H, W) != self.heatmap_size:
            raise ValueError(f"PoseEvalStep: heatmaps are {H}x{W}, heatmap_size is {self.heatmap_size}")
        if K != len(self.kp_weights):
            raise ValueError(f"PoseEvalStep: {K} heatmap channels, {len(self.kp_weights)} keypoint weights")
        dev = heatmaps.device
        kp, boxes, areas = (batch[k].to(dev, torch.float32) for k in ("keypoints", "boxes", "areas"))
        N = kp.shape[1]
        if self._state is None:
            self._state = (torch.zeros(1, dtype=torch.int64, device=dev),
                           torch.empty(self.capacity, K, 3, device=dev), torch.empty(self.capacity, 8, device=dev))
        slot_base = len(self._slot_ids)
        keep = self.keep_flags(batch["image_ids"], commit=False)
        if len(keep) != B:
            raise ValueError(f"PoseEvalStep: {len(keep)} image ids for {B} frames")
        out = ops.pose_eval_loss(heatmaps, kp, self.kp_weights, heat_flipped=heatmaps_flipped,
                                 partner=flip_partner(K), mode=0 if self.flip_mode == "reference" else 1,
                                 areas=areas, boxes=boxes, sigma=self.sigma, topk=self.ohkm_topk)
        ops.pose_coco_records(out["coords"], out["scores"], boxes, areas, batch["masks"].to(dev),
                              batch["is_crowd"].to(dev), keep, self.keypoint_thresh, slot_base, *self._state)
        self.keep_flags(batch["image_ids"])           # both launches are queued: the ids are now seen
        self._max_records += sum(keep) * N
        self.last = out
        return out["loss"][0]

    def compute(self, gt: CocoKeypointGT) -> dict:
        """on_validation_epoch_end's metrics (module.py:600-622) of the epoch's records against
        ``gt``: COCOeval's evaluate / accumulate / summarize on the device. One small upload (the
        slots' rows in ``gt``) and one read (the ten numbers and the record counter).
        ``self.last_eval`` keeps the device tensors (precision, recall, oks, dt_bits, ...)."""
        K = len(self.kp_weights)
        if gt.K != K:
            raise ValueError(f"PoseEvalStep.compute: the annotations have {gt.K} keypoints, the records {K}")
        if self._state is None:
            dev = torch.device(self.device)
            counter, kpts, meta = None, torch.empty(0, K, 3, device=dev), torch.empty(0, 8, device=dev)
        else:
            counter, kpts, meta = self._state
        n = min(self._max_records, kpts.shape[0])
        ev = coco_keypoint_eval(kpts, meta, counter, n, self._slot_ids, gt)
        tail = ev["stats"] if counter is None else torch.cat([ev["stats"], counter.view(torch.float64)])
        host = tail.cpu().numpy()
        count = 0 if counter is None else int(host[10:].view(np.int64)[0])
        if count > self.capacity:
            raise RuntimeError(f"PoseEvalStep: {count} records exceed the capacity {self.capacity}")
        self.last_eval = ev
        return dict(zip(COCO_KP_STAT_KEYS, host[:10].tolist()))

    def predictions(self) -> list[dict]:
        """The epoch's eval_predictions (module.py:552-561), one device-to-host read."""
        if self._state is None:
            return []
        counter, kpts, meta = self._state
        n = min(self._max_records, self.capacity)
        K = kpts.shape[1]
        flat = torch.cat([kpts[:n].reshape(-1), meta[:n].reshape(-1), counter.view(torch.float32)]).cpu().numpy()
        count = int(flat[-2:].view(np.int64)[0])
        if count > self.capacity:
            raise RuntimeError(f"PoseEvalStep: {count} records exceed the capacity {self.capacity}")
        return format_coco_records(flat[:n * K * 3].reshape(n, K, 3)[:count],
                                   flat[n * K * 3:n * (K * 3 + 8)].reshape(n, 8)[:count], self._slot_ids)
