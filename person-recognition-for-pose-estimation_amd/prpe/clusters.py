"""Clustering of unlabelled face embeddings (csrc/facecluster.hip behind
prpe_pair_degree / prpe_pair_link / prpe_cluster_finish / prpe_cluster_centroids).

* ``FaceClusters``   — a store of normalised embeddings without labels (a ``FaceGallery``: its own,
  or an existing one through ``of_gallery``). ``cluster`` groups the rows into identities by DBSCAN
  over the cosine score on the device (the score matrix is never stored; no host read).
* ``FaceClustering`` — the result, device tensors. ``enrol_into`` appends one template per cluster
  to a gallery, so the next frame recognises the person: the one host read.

A score is the one ``FaceGallery.identify`` compares, so "two rows are linked at threshold t" means
"``identify`` would accept one as the other at t", and a threshold from ``FaceIdentifier.calibrate``
serves unchanged. The reference has no clustering code; the semantics are stated in include/prpe.h.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import ops
from .gallery import FaceGallery


@dataclass
class FaceClustering:
    """Device tensors of one ``FaceClusters.cluster`` call (include/prpe.h): root, kind (0 left out,
    1 noise, 2 border, 3 core), degree and cluster per row; n_clusters [1]; sizes, sums (int64
    fixed point), centroids_raw (the member sums, not normalised), centroids (normalised by
    ops.gallery_enrol) and centroid_norms per cluster, [max_clusters] rows of which the first
    min(n_clusters, max_clusters) are meaningful."""
    root: torch.Tensor
    kind: torch.Tensor
    degree: torch.Tensor
    cluster: torch.Tensor
    n_clusters: torch.Tensor
    sizes: torch.Tensor
    sums: torch.Tensor
    centroids_raw: torch.Tensor
    centroids: torch.Tensor
    centroid_norms: torch.Tensor
    threshold: float
    min_samples: int

    @property
    def max_clusters(self):
        return self.sizes.numel()

    def enrol_into(self, gallery: FaceGallery, first_label: int, min_size: int = 1):
        """Append the centroid of every cluster with at least ``min_size`` members to ``gallery``
        as identity ``first_label + cluster id``; returns ((first, last + 1) rows, labels). This is
        the one host read of the clustering (n_clusters and sizes). Raises, leaving the gallery as
        it was, past the gallery's capacity or when n_clusters exceeded max_clusters (the clusters
        past it have no centroid)."""
        if not isinstance(gallery, FaceGallery) or gallery.dim != self.centroids_raw.shape[1]:
            raise ValueError(f"FaceClustering.enrol_into: expected a FaceGallery of dim {self.centroids_raw.shape[1]}")
        host = torch.cat([self.n_clusters, self.sizes]).cpu()
        C = int(host[0])
        if C > self.max_clusters:
            raise ValueError(f"FaceClustering.enrol_into: {C} clusters exceeded max_clusters = {self.max_clusters}")
        ids = [c for c in range(C) if int(host[1 + c]) >= int(min_size)]
        n = len(gallery)
        if not ids:
            return (n, n), []
        if n + len(ids) > gallery.capacity:
            raise ValueError(f"FaceClustering.enrol_into: {n} + {len(ids)} rows exceed the capacity {gallery.capacity}")
        labels = [int(first_label) + c for c in ids]
        index = torch.tensor(ids, dtype=torch.int64).to(self.centroids_raw.device)
        return gallery.add(self.centroids_raw.index_select(0, index), labels), labels


class FaceClusters:
    def __init__(self, dim: int = 512, capacity: int = 4096, device="cuda", _store=None):
        self.store = _store if _store is not None else FaceGallery(dim=dim, capacity=capacity, device=device)
        self.dim, self.device = self.store.dim, self.store.device

    @classmethod
    def of_gallery(cls, gallery: FaceGallery):
        """A view of ``gallery``'s rows and valid bytes (no copy; later ``add`` / ``remove`` on the
        gallery show; its labels play no role): duplicate identities and mislabelled rows of what
        has been enrolled show as clusters that disagree with the labels."""
        if not isinstance(gallery, FaceGallery):
            raise ValueError("FaceClusters.of_gallery: expected a FaceGallery")
        return cls(_store=gallery)

    def __len__(self):
        return len(self.store)

    def add(self, embeddings):
        """Append raw ``embeddings`` [n, dim]: ``FaceGallery.add``'s contract with label 0
        (normalised by ops.gallery_enrol, raises past the capacity, nothing read back)."""
        n = embeddings.shape[0] if isinstance(embeddings, torch.Tensor) and embeddings.dim() == 2 else 0
        return self.store.add(embeddings, [0] * n)

    def add_frames(self, identifier, frames):
        return self.add(identifier.embed(frames))

    def add_frames_u8(self, identifier, frames_u8, ingest=None):
        return self.add(identifier.embed_u8(frames_u8, ingest))

    def cluster(self, threshold: float, min_samples: int = 2, max_clusters=None) -> FaceClustering:
        """DBSCAN over the cosine score of the stored rows (include/prpe.h): rows scoring at least
        ``threshold`` are neighbours, a row with ``min_samples`` rows in its neighbourhood (itself
        included) is core. ``max_clusters`` None: ``len(self)``, which no clustering exceeds.
        Everything stays on the device; no host read."""
        n = len(self.store)
        if n < 1:
            raise ValueError("FaceClusters.cluster: no rows")
        max_clusters = n if max_clusters is None else int(max_clusters)
        if max_clusters < 1:
            raise ValueError(f"FaceClusters.cluster: max_clusters must be at least 1, got {max_clusters}")
        a, valid, dev, D = self.store.rows[:n], self.store.valid[:n], self.device, self.dim
        degree = torch.empty(n, device=dev, dtype=torch.int32)
        root, cluster = torch.empty_like(degree), torch.empty_like(degree)
        kind = torch.empty(n, device=dev, dtype=torch.uint8)
        n_clusters = torch.empty(1, device=dev, dtype=torch.int32)
        sizes = torch.zeros(max_clusters, device=dev, dtype=torch.int32)
        sums = torch.zeros(max_clusters, D, device=dev, dtype=torch.int64)
        raw = torch.zeros(max_clusters, D, device=dev, dtype=torch.float32)
        workspace = torch.empty(ops.face_cluster_workspace_bytes(n), device=dev, dtype=torch.uint8)
        ops.pair_degree(a, threshold, degree=degree, valid=valid)
        ops.pair_link(a, threshold, min_samples, degree=degree, workspace=workspace, valid=valid)
        ops.cluster_finish(n, min_samples, degree=degree, workspace=workspace, root=root, kind=kind, cluster=cluster,
                           n_clusters=n_clusters, sizes=sizes, valid=valid)
        ops.cluster_centroids(a, cluster=cluster, n_clusters=n_clusters, sums=sums, centroids=raw)
        unit = torch.zeros_like(raw)
        norms = torch.zeros(max_clusters, device=dev, dtype=torch.float32)
        ops.gallery_enrol(raw, unit, norms, 0)
        return FaceClustering(root=root, kind=kind, degree=degree, cluster=cluster, n_clusters=n_clusters, sizes=sizes,
                              sums=sums, centroids_raw=raw, centroids=unit, centroid_norms=norms,
                              threshold=float(threshold), min_samples=int(min_samples))
