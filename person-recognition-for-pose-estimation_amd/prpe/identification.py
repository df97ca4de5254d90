"""Open-set 1:N identification evaluation of a gallery against a labelled probe set (DESIGN.md §5p;
csrc/identeval.hip behind prpe_ident_best / prpe_ident_rank / prpe_ident_finish).

* ``IdentificationEval`` — a probe store (a ``FaceGallery``, as ``FaceVerification`` has one)
  beside the gallery under test. ``evaluate`` finds on the device, per probe, the best enrolled row
  of its own label, the best row of any other label and the rank of the first mate, and bins the
  probes; the score matrix is never stored and nothing is read back. ``compute`` reads the
  histograms once and derives DIR / FNIR / FPIR per threshold, the thresholds at requested FPIR
  and the CMC on the host in integers and fp64. ``leave_one_out`` evaluates a gallery on its own
  rows, each against all others.
* ``identification_curve`` — that host part, on the histograms.

A score is the one ``FaceGallery.identify`` compares and a bin edge is exact in fp32, so the sums
over the bins at and above an edge ARE the probes ``identify`` names rightly, wrongly, and names
although they are strangers, at that threshold (include/prpe.h). Unlike the pairwise FAR of
``FaceVerification``, the FPIR is a rate per identify call on the gallery as it is enrolled. The
reference has no such code; the semantics are this project's.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .gallery import FaceGallery
from .verification import bin_edges


def identification_curve(hist, rank_hist, counts, fpir=(1e-1, 1e-2, 1e-3)) -> dict:
    """The curves of ``prpe_ident_finish``'s outputs: hist [3, nbins] (row 0 right label, row 1
    wrong label, row 2 stranger named), rank_hist [ranks + 1] (None: no CMC) and counts [4] (mated,
    non-mated, left out, without any candidate). Per edge b = 0..nbins, with S_r[b] the sum of
    row r over the bins >= b (exact integers): DIR = S_0 / mated, wrong = S_1 / mated,
    FNIR = 1 - DIR, FPIR = S_2 / non-mated; per requested FPIR the lowest edge with
    S_2[b] <= fpir * non-mated; CMC[r - 1] = mated probes of rank <= r / mated. NaN where a
    denominator is 0; nothing raises."""
    hist = np.asarray(hist).astype(np.int64).reshape(3, -1)
    counts = np.asarray(counts).astype(np.int64).reshape(4)
    nbins = hist.shape[1]
    zero = np.zeros((3, 1), dtype=np.int64)
    S = np.concatenate([np.cumsum(hist[:, ::-1], axis=1)[:, ::-1], zero], axis=1)
    mated, nonmated = int(counts[0]), int(counts[1])
    thr = bin_edges(nbins)
    nan = np.full(nbins + 1, np.nan)
    dir_ = S[0] / mated if mated else nan
    wrong = S[1] / mated if mated else nan
    fp = S[2] / nonmated if nonmated else nan
    rows = []
    for f in fpir:
        f = float(f)
        ok = S[2].astype(np.float64) <= f * float(nonmated)                   # S_2[nbins] = 0 meets every f >= 0
        b = int(np.argmax(ok)) if ok.any() else nbins
        rows.append({"fpir": f, "bin": b, "threshold": float(thr[b]), "dir": float(dir_[b]), "fnir": float(1 - dir_[b]),
                     "wrong": float(wrong[b]), "false_positives": int(S[2][b]), "right_names": int(S[0][b]),
                     "wrong_names": int(S[1][b])})
    out = {"mated": mated, "non_mated": nonmated, "left_out": int(counts[2]), "no_candidate": int(counts[3]),
           "nbins": nbins, "at_fpir": rows, "hist": hist,
           "curve": {"thresholds": thr, "dir": dir_, "wrong": wrong, "fnir": 1 - dir_, "fpir": fp},
           "cmc": None, "beyond_cmc": None}
    if rank_hist is not None:
        rank_hist = np.asarray(rank_hist).astype(np.int64).reshape(-1)
        hits = np.cumsum(rank_hist[:-1])
        out["cmc"] = hits / mated if mated else np.full(hits.shape, np.nan)
        out["beyond_cmc"] = int(rank_hist[-1])
    return out


class IdentificationEval:
    def __init__(self, gallery: FaceGallery, capacity: int = 4096, _probes=None):
        if not isinstance(gallery, FaceGallery):
            raise ValueError("IdentificationEval: expected a FaceGallery")
        self.gallery = gallery
        self.dim, self.device = gallery.dim, gallery.device
        self.self_mode = _probes is gallery
        self.probes = _probes if _probes is not None else FaceGallery(dim=self.dim, capacity=capacity,
                                                                      device=self.device)

    @classmethod
    def leave_one_out(cls, gallery: FaceGallery):
        """Self mode on ``gallery``'s own rows (no copy): every enrolled row is a probe against all
        other rows, so a row whose identity has no second row is a stranger."""
        return cls(gallery, _probes=gallery)

    def __len__(self):
        return len(self.probes)

    def add(self, embeddings, labels):
        """Append raw probe ``embeddings`` [n, dim] with their true ``labels``: ``FaceGallery.add``'s
        contract. A label the gallery does not hold makes the probe a stranger."""
        if self.self_mode:
            raise ValueError("IdentificationEval.add: a leave-one-out evaluation has no probe store")
        return self.probes.add(embeddings, labels)

    def add_frames(self, identifier, frames, labels):
        return self.add(identifier.embed(frames), labels)

    def add_frames_u8(self, identifier, frames_u8, labels, ingest=None):
        return self.add(identifier.embed_u8(frames_u8, ingest), labels)

    @staticmethod
    def _operands(store, what):
        n = len(store)
        if n < 1:
            raise ValueError(f"IdentificationEval.evaluate: no {what}")
        return store.rows[:n], store.labels[:n], store.valid[:n]

    def evaluate(self, nbins: int = 2048, cmc: bool = True) -> dict:
        """The passes on the device, no host read. Returns the device tensors mate_key, non_key
        (int64 [M] holding the keys), mate_score, non_score, mate_row, non_row, rank [M],
        hist [3, nbins], counts [4], skipped [1] and, with ``cmc``, rank_minus_1 [M] and
        rank_hist [65] (include/prpe.h). Without ``cmc`` the second pass is not run and rank is
        1, 0 or -1 (above 1)."""
        a, la, va = self._operands(self.probes, "probes")
        M, dev = a.shape[0], self.device
        cross = {}
        if not self.self_mode:
            b, lb, vb = self._operands(self.gallery, "gallery rows")
            cross = {"b": b, "b_labels": lb, "b_valid": vb}
        z64 = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.int64)
        i32 = lambda: torch.empty(M, device=dev, dtype=torch.int32)
        f32 = lambda: torch.empty(M, device=dev, dtype=torch.float32)
        out = {"mate_key": z64(M), "non_key": z64(M), "skipped": z64(1), "hist": z64(3, int(nbins)), "counts": z64(4),
               "mate_score": f32(), "non_score": f32(), "mate_row": i32(), "non_row": i32(), "rank": i32(),
               "rank_minus_1": None, "rank_hist": None}
        ops.ident_best(a, la, mate_key=out["mate_key"], non_key=out["non_key"], skipped=out["skipped"], a_valid=va,
                       **cross)
        if cmc:
            out["rank_minus_1"] = torch.zeros(M, device=dev, dtype=torch.int32)
            out["rank_hist"] = z64(ops.IDENT_RANKS + 1)
            ops.ident_rank(a, la, mate_key=out["mate_key"], rank_minus_1=out["rank_minus_1"], a_valid=va, **cross)
        ops.ident_finish(la, mate_key=out["mate_key"], non_key=out["non_key"], nbins=nbins, a_valid=va,
                         rank_minus_1=out["rank_minus_1"], rank_hist=out["rank_hist"],
                         **{k: out[k] for k in ("mate_score", "mate_row", "non_score", "non_row", "rank", "hist",
                                                "counts")})
        return out

    def compute(self, nbins: int = 2048, fpir=(1e-1, 1e-2, 1e-3), cmc: bool = True) -> dict:
        """``evaluate`` and ``identification_curve`` of it: one host read of at most 100 KB."""
        dev = self.evaluate(nbins, cmc)
        parts = [dev["hist"].reshape(-1), dev["counts"], dev["skipped"]] + ([dev["rank_hist"]] if cmc else [])
        host = torch.cat(parts).cpu().numpy()
        n = 3 * int(nbins)
        out = identification_curve(host[:n].reshape(3, -1), host[n + 5:] if cmc else None, host[n:n + 4], fpir)
        out["skipped"] = int(host[n + 4])
        return out
