"""1:1 face verification over all pairs of a labelled embedding set (DESIGN.md §5i;
csrc/pairhist.hip behind prpe_pair_hist).

* ``FaceVerification`` — a store of normalised embeddings with labels (a ``FaceGallery``: its own,
  or an existing one through ``of_gallery``). ``histogram`` bins the cosine score of every pair
  into a genuine and an impostor histogram on the device (the score matrix is never stored; no
  host read); ``compute`` reads the two histograms once and derives the ROC, TAR at fixed FAR, the
  EER and the best-accuracy threshold on the host in integers and fp64.
* ``verification_curve`` — that host part, on a histogram.

A score is the one ``FaceGallery.identify`` compares, and a bin edge is exact in fp32, so the
impostor count at and above an edge IS the number of pairs ``identify`` accepts at that threshold
(include/prpe.h). The reference has no verification code; the semantics are this project's.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .gallery import FaceGallery


def bin_edges(nbins: int):
    """thresholds [nbins + 1] fp64: accepting ``score >= thresholds[b]`` accepts exactly the pairs of
    the bins >= b. edge_b = (b - h) / h inside; -inf at b = 0 and +inf at b = nbins, because the
    two outer bins are clamped (the top bin holds every score >= edge_{nbins-1}, also one above 1)."""
    h = nbins // 2
    t = (np.arange(nbins + 1, dtype=np.float64) - h) / h
    t[0], t[nbins] = -np.inf, np.inf
    return t


def verification_curve(hist, far=(1e-1, 1e-2, 1e-3, 1e-4), skipped=0) -> dict:
    """The curve of a [2, nbins] histogram (row 0 genuine, row 1 impostor); see DESIGN.md §5i.
    TA[b] / FA[b] = the genuine / impostor pairs in the bins >= b, b = 0..nbins (exact integers);
    TAR = TA / genuine, FAR = FA / impostor (NaN without such pairs; nothing raises)."""
    hist = np.asarray(hist).astype(np.int64).reshape(2, -1)
    nbins = hist.shape[1]
    zero = np.zeros((2, 1), dtype=np.int64)
    acc = np.concatenate([np.cumsum(hist[:, ::-1], axis=1)[:, ::-1], zero], axis=1)
    TA, FA = acc[0], acc[1]
    genuine, impostor = int(TA[0]), int(FA[0])
    thr = bin_edges(nbins)
    nan = np.full(nbins + 1, np.nan)
    tar = TA / genuine if genuine else nan
    farc = FA / impostor if impostor else nan
    rows = []
    for f in far:
        f = float(f)
        if not 0.0 <= f <= 1.0:
            raise ValueError(f"verification_curve: a false-accept rate lies in [0, 1], got {f}")
        b = int(np.argmax(FA.astype(np.float64) <= f * float(impostor)))     # FA[nbins] = 0 always meets it
        rows.append({"far": f, "bin": b, "threshold": float(thr[b]), "tar": float(tar[b]),
                     "false_accepts": int(FA[b]), "true_accepts": int(TA[b])})
    out = {"genuine": genuine, "impostor": impostor, "skipped": int(skipped), "nbins": nbins, "at_far": rows,
           "roc": {"thresholds": thr, "tar": tar, "far": farc}, "hist": hist,
           "eer": float("nan"), "eer_threshold": float("nan"),
           "best_accuracy": float("nan"), "best_threshold": float("nan")}
    if genuine and impostor:
        b = int(np.argmin(np.abs(farc - (1 - tar))))                         # the lowest b on ties
        out["eer"], out["eer_threshold"] = float((farc[b] + 1 - tar[b]) / 2), float(thr[b])
    if genuine + impostor:
        correct = TA + (impostor - FA)
        b = int(np.argmax(correct))                                          # the lowest b on ties
        out["best_accuracy"], out["best_threshold"] = float(correct[b] / (genuine + impostor)), float(thr[b])
    return out


class FaceVerification:
    def __init__(self, dim: int = 512, capacity: int = 4096, device="cuda", _store=None):
        self.store = _store if _store is not None else FaceGallery(dim=dim, capacity=capacity, device=device)
        self.dim, self.device = self.store.dim, self.store.device

    @classmethod
    def of_gallery(cls, gallery: FaceGallery):
        """A view of ``gallery``'s rows, labels and valid bytes (no copy; later ``add`` / ``remove``
        on the gallery show): how separable is what has been enrolled?"""
        if not isinstance(gallery, FaceGallery):
            raise ValueError("FaceVerification.of_gallery: expected a FaceGallery")
        return cls(_store=gallery)

    def __len__(self):
        return len(self.store)

    def add(self, embeddings, labels):
        """Append raw ``embeddings`` [n, dim] with ``labels``: ``FaceGallery.add``'s contract
        (normalised by ops.gallery_enrol, raises past the capacity, nothing read back)."""
        return self.store.add(embeddings, labels)

    def add_frames(self, identifier, frames, labels):
        return self.add(identifier.embed(frames), labels)

    def add_frames_u8(self, identifier, frames_u8, labels, ingest=None):
        return self.add(identifier.embed_u8(frames_u8, ingest), labels)

    @staticmethod
    def _operands(what, store):
        n = len(store)
        if n < 1:
            raise ValueError(f"FaceVerification.{what}: no rows")
        return store.rows[:n], store.labels[:n], store.valid[:n]

    def histogram(self, nbins: int = 2048, against=None):
        """(hist int64 [2, nbins], skipped int64 [1]) on the device, no host read: all pairs i < j
        of this set, or with ``against`` (a ``FaceGallery`` or ``FaceVerification``) all pairs of a
        row here and a row there. Removed rows (valid byte 0) and labels < 0 take part in no pair."""
        a, la, va = self._operands("histogram", self.store)
        hist = torch.zeros(2, int(nbins), device=self.device, dtype=torch.int64)
        skipped = torch.zeros(1, device=self.device, dtype=torch.int64)
        if against is None:
            ops.pair_hist(a, la, nbins=nbins, hist=hist, skipped=skipped, a_valid=va)
        else:
            other = against.store if isinstance(against, FaceVerification) else against
            if not isinstance(other, FaceGallery) or other.dim != self.dim:
                raise ValueError(f"FaceVerification.histogram: against must be a FaceGallery or FaceVerification "
                                 f"of dim {self.dim}")
            b, lb, vb = self._operands("histogram", other)
            ops.pair_hist(a, la, b, lb, nbins=nbins, hist=hist, skipped=skipped, a_valid=va, b_valid=vb)
        return hist, skipped

    def compute(self, nbins: int = 2048, far=(1e-1, 1e-2, 1e-3, 1e-4), against=None) -> dict:
        """``histogram`` and ``verification_curve`` of it: one host read of at most 64 KB."""
        hist, skipped = self.histogram(nbins, against)
        host = torch.cat([hist.reshape(-1), skipped]).cpu().numpy()
        return verification_curve(host[:-1].reshape(2, -1), far, skipped=int(host[-1]))
