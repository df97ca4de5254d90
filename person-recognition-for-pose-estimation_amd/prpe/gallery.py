"""Face identification: the enrolled gallery and the stage that matches embeddings against it
(csrc/gallery.hip behind prpe_gallery_enrol / prpe_gallery_topk).

* ``FaceGallery``    — normalised embeddings, their norms, an int64 label and a valid byte per row,
  all on the device. ``add`` appends (the size is a host integer: nothing is read back),
  ``remove`` clears valid bytes with elementwise device ops, ``search`` is the fused cosine top-k,
  ``identify`` the top-1 with a rejection threshold. No call synchronises with the host.
  ``route`` ("exact", "wide" or "auto") chooses between the exact search and the wide-batch route
  of DESIGN.md §5k, which returns the same bits and is faster for many queries per call.
* ``FaceIdentifier`` — frames -> trunk -> AdaFace embedding -> ``add`` / ``identify``; it calls the
  engine directly, so the model's ``set_task`` state is left alone. ``calibrate`` takes its
  threshold from a ``FaceVerification`` (prpe/verification.py) at a target FAR,
  ``calibrate_fpir`` from an ``IdentificationEval`` (prpe/identification.py, §5p) at a target
  false-positive identification rate on the gallery as enrolled.

The reference names the task (scripts/modify_models.py:331) but has no gallery code; the semantics
are stated in include/prpe.h.
"""
from __future__ import annotations

import torch

from . import ops


class FaceGallery:
    def __init__(self, dim: int = 512, capacity: int = 4096, device="cuda", route: str = "exact"):
        dim, capacity = int(dim), int(capacity)
        ops.gallery_route(route, 1, 1)
        self.route = route
        if dim % 32 or not 32 <= dim <= ops.GALLERY_MAX_DIM:
            raise ValueError(f"FaceGallery: dim must be a multiple of 32 in [32, {ops.GALLERY_MAX_DIM}], got {dim}")
        if capacity < 1:
            raise ValueError(f"FaceGallery: capacity must be at least 1, got {capacity}")
        self.dim, self.capacity, self.device = dim, capacity, torch.device(device)
        self.rows = torch.zeros(capacity, dim, device=self.device, dtype=torch.float32)
        self.norms = torch.zeros(capacity, device=self.device, dtype=torch.float32)
        self.labels = torch.full((capacity,), -1, device=self.device, dtype=torch.int64)
        self.valid = torch.zeros(capacity, device=self.device, dtype=torch.uint8)
        self._size = 0

    def __len__(self):
        """Rows enrolled so far, removed ones included (a host integer)."""
        return self._size

    def reset(self):
        self._size = 0
        self.valid.zero_()
        self.labels.fill_(-1)

    def _embeddings(self, what, e):
        if not (isinstance(e, torch.Tensor) and e.is_cuda and e.dim() == 2 and e.shape[1] == self.dim and
                e.shape[0] >= 1):
            raise ValueError(f"FaceGallery.{what}: embeddings must be a device tensor [n >= 1, {self.dim}]")
        return e.to(torch.float32).contiguous()

    def add(self, embeddings, labels):
        """Append ``embeddings`` [n, dim] with ``labels`` (int64 [n] device tensor, or host integers).
        Raises past the capacity and leaves the gallery as it was. Returns the (first, last + 1) rows."""
        e = self._embeddings("add", embeddings)
        n = e.shape[0]
        lab = torch.as_tensor(labels, dtype=torch.int64).to(self.device).reshape(-1)
        if lab.numel() != n:
            raise ValueError(f"FaceGallery.add: {n} embeddings with {lab.numel()} labels")
        if self._size + n > self.capacity:
            raise ValueError(f"FaceGallery.add: {self._size} + {n} rows exceed the capacity {self.capacity}")
        a, b = self._size, self._size + n
        ops.gallery_enrol(e, self.rows, self.norms, a)
        self.labels[a:b] = lab
        self.valid[a:b] = 1
        self._size = b
        return a, b

    def remove(self, labels):
        """Every enrolled row whose label is in ``labels`` stops matching (its valid byte is cleared;
        the row keeps its place, so the indices of the others do not move)."""
        lab = torch.as_tensor(labels, dtype=torch.int64).to(self.device).reshape(-1)
        if self._size and lab.numel():
            hit = torch.isin(self.labels[:self._size], lab)
            self.valid[:self._size] &= (~hit).to(torch.uint8)

    def _require_rows(self, what):
        if self._size < 1:
            raise ValueError(f"FaceGallery.{what}: the gallery is empty")

    def _topk(self, route, Q):
        """ops.gallery_topk or ops.gallery_topk_wide: ``route`` (None: the gallery's own setting) is
        "exact", "wide" or "auto" (wide from ops.GALLERY_WIDE_MIN_Q queries and ops.GALLERY_WIDE_MIN_G
        enrolled rows on). Both give the same bits."""
        taken = ops.gallery_route(self.route if route is None else route, Q, self._size)
        return ops.gallery_topk_wide if taken == "wide" else ops.gallery_topk

    def search(self, embeddings, k: int = 5, route=None):
        """(scores [Q, k], rows [Q, k] int32, labels [Q, k] int64): the k best enrolled rows per
        embedding by cosine similarity, descending (ties: the lower row); rows / labels -1 and score
        -inf where fewer than k rows are valid. ``route`` overrides the gallery's setting for this call."""
        self._require_rows("search")
        e = self._embeddings("search", embeddings)
        Q = e.shape[0]
        scores = torch.empty(Q, k, device=self.device, dtype=torch.float32)
        rows = torch.empty(Q, k, device=self.device, dtype=torch.int32)
        self._topk(route, Q)(e, self.rows, self._size, k, scores=scores, rows=rows, valid=self.valid)
        lab = torch.where(rows >= 0, self.labels[rows.clamp(min=0).long()], torch.full_like(rows, -1, dtype=torch.int64))
        return scores, rows, lab

    def identify(self, embeddings, threshold: float, route=None):
        """(ident [Q] int64, score [Q]): the label of the best valid row when its cosine similarity
        is at least ``threshold``, else -1; score is that best similarity (-inf with no valid row).
        ``route`` overrides the gallery's setting for this call."""
        self._require_rows("identify")
        e = self._embeddings("identify", embeddings)
        Q = e.shape[0]
        scores = torch.empty(Q, 1, device=self.device, dtype=torch.float32)
        rows = torch.empty(Q, 1, device=self.device, dtype=torch.int32)
        ident = torch.empty(Q, device=self.device, dtype=torch.int64)
        self._topk(route, Q)(e, self.rows, self._size, 1, scores=scores, rows=rows, valid=self.valid,
                             labels=self.labels, threshold=float(threshold), ident=ident)
        return ident, scores.view(Q)


class FaceIdentifier:
    """``enrol(frames, labels)`` / ``identifier(frames)`` -> (ident, score) through the model's
    face-recognition branch (trunk -> IR-50 -> 512-d embedding) and a ``FaceGallery``."""

    def __init__(self, model, gallery: FaceGallery, threshold: float = 0.3):
        if gallery.dim != 512:
            raise ValueError(f"FaceIdentifier: the AdaFace embedding is 512-d, the gallery holds {gallery.dim}")
        self.model, self.gallery, self.threshold = model, gallery, float(threshold)

    @torch.no_grad()
    def embed(self, frames):
        m = self.model
        x = m._check_input(frames)
        m._sync_weights()
        emb, _ = m.engine.adaface(m.engine.trunk(x))
        return emb

    @torch.no_grad()
    def embed_u8(self, frames_u8, ingest=None):
        """``embed`` on uint8 source frames: a tensor [B, Hs, Ws, 3], or a sequence of frames
        [Hs_i, Ws_i, 3] of different sizes (``CombinedModel.forward_u8``)."""
        m = self.model
        frames_u8, ingest = m._check_input_u8(frames_u8, ingest, sequence=True)
        m._sync_weights()
        emb, _ = m.engine.adaface(m.engine.trunk_u8(frames_u8, ingest))
        return emb

    def enrol(self, frames, labels):
        return self.gallery.add(self.embed(frames), labels)

    def enrol_u8(self, frames_u8, labels, ingest=None):
        return self.gallery.add(self.embed_u8(frames_u8, ingest), labels)

    def __call__(self, frames):
        return self.gallery.identify(self.embed(frames), self.threshold)

    def calibrate(self, verification, far: float):
        """Set ``threshold`` to the lowest bin edge at which the impostor pairs of ``verification``
        (a ``prpe.FaceVerification``) are accepted at a rate of at most ``far``; returns that row of
        ``verification.compute`` (threshold, tar, false_accepts, true_accepts). One host read."""
        row = verification.compute(far=(far,))["at_far"][0]
        self.threshold = float(row["threshold"])
        return row

    def calibrate_fpir(self, evaluation, fpir: float):
        """Set ``threshold`` to the lowest bin edge at which the strangers among ``evaluation``'s
        probes (a ``prpe.IdentificationEval`` on the enrolled gallery) are named at a rate of at most
        ``fpir`` per identify call; returns that row of ``evaluation.compute`` (threshold, dir, fnir,
        false_positives, right_names, wrong_names). One host read."""
        row = evaluation.compute(fpir=(fpir,), cmc=False)["at_fpir"][0]
        self.threshold = float(row["threshold"])
        return row

    def from_frames_u8(self, frames_u8, ingest=None):
        """``__call__`` on uint8 source frames [B, Hs, Ws, 3] through ``trunk_u8`` (prpe.FrameIngest)."""
        return self.gallery.identify(self.embed_u8(frames_u8, ingest), self.threshold)
