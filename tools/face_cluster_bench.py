"""Time the stages of the on-device face clustering (prpe_pair_degree, prpe_pair_link,
prpe_cluster_finish, prpe_cluster_centroids) with prpe_pair_hist on the same rows as the yardstick
(DESIGN.md §5j).

    python tools/face_cluster_bench.py [--n 4096 32768] [--iters 20] [--far 1e-3]

D = 512, 1000 planted identities (a unit-variance centre per identity plus unit-variance noise),
min_samples = 2, the threshold taken from FaceVerification.compute at the given FAR on the same
rows. Each GEMM pass does pair_hist's matrix work (the upper triangle of 128 x 128 tiles), so the
number to read is pass time / pair_hist time. A second set per N holds one identity only (every
pair an edge): the worst case for pass 2's union-find.
HIP-event timing, 3 warm-ups per stage, the stages alternated inside each iteration, medians with
(min, max). One JSON line per case. exec_TFps = the executed fp32-MFMA FLOP of a GEMM pass
(2 T^2 D per tile) / median.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pair_hist_bench import D, PEAK_TF, timed  # noqa: E402
from prpe import FaceGallery, FaceVerification, ops  # noqa: E402


def bench(rows, labels, threshold, min_samples, iters):
    N, dev = rows.shape[0], rows.device
    degree = torch.empty(N, device=dev, dtype=torch.int32)
    root, cluster = torch.empty_like(degree), torch.empty_like(degree)
    kind = torch.empty(N, device=dev, dtype=torch.uint8)
    n_clusters = torch.empty(1, device=dev, dtype=torch.int32)
    sizes = torch.zeros(N, device=dev, dtype=torch.int32)
    sums = torch.zeros(N, D, device=dev, dtype=torch.int64)
    centroids = torch.zeros(N, D, device=dev)
    ws = torch.empty(ops.face_cluster_workspace_bytes(N), device=dev, dtype=torch.uint8)
    hist = torch.zeros(2, 2048, device=dev, dtype=torch.int64)
    skipped = torch.zeros(1, device=dev, dtype=torch.int64)
    # every stage reads what the stage before it left, so the order inside an iteration is the pipeline's
    stages = {
        "pair_hist": lambda: ops.pair_hist(rows, labels, nbins=2048, hist=hist, skipped=skipped),
        "degree": lambda: ops.pair_degree(rows, threshold, degree=degree),
        "link": lambda: ops.pair_link(rows, threshold, min_samples, degree=degree, workspace=ws),
        "finish": lambda: ops.cluster_finish(N, min_samples, degree=degree, workspace=ws, root=root, kind=kind,
                                             cluster=cluster, n_clusters=n_clusters, sizes=sizes),
        "centroids": lambda: ops.cluster_centroids(rows, cluster=cluster, n_clusters=n_clusters, sums=sums,
                                                   centroids=centroids),
    }
    for f in stages.values():          # once in order, so that the warm-ups of a later stage read real inputs
        f()
    t = timed(stages, iters)
    torch.cuda.synchronize()
    tiles = -(-N // ops.PAIR_HIST_TILE)
    flop = 2.0 * (tiles * (tiles + 1) // 2) * ops.PAIR_HIST_TILE ** 2 * D
    out = {k: v for k, v in t.items()}
    out["sum_ms"] = round(sum(t[k]["ms"] for k in ("degree", "link", "finish", "centroids")), 4)
    for k in ("degree", "link"):
        out[k + "_over_pair_hist"] = round(t[k]["ms"] / t["pair_hist"]["ms"], 3)
        out[k + "_exec_TFps"] = round(flop / t[k]["ms"] / 1e9, 2)
    out["pair_hist_exec_TFps"] = round(flop / t["pair_hist"]["ms"] / 1e9, 2)
    out["peak_TFps"] = PEAK_TF
    kinds = torch.bincount(kind.long(), minlength=4).tolist()
    out.update(clusters=int(n_clusters[0]), kinds=kinds, edges=int(degree.long().sum()) // 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--identities", type=int, default=1000)
    ap.add_argument("--far", type=float, default=1e-3)
    ap.add_argument("--min-samples", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "face_cluster_bench needs the MI355X"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    for N in a.n:
        labels = torch.randint(0, a.identities, (N,), device=dev, generator=gen)
        gal = FaceGallery(dim=D, capacity=N, device=dev)
        gal.add(torch.randn(a.identities, D, device=dev, generator=gen)[labels] +
                torch.randn(N, D, device=dev, generator=gen), labels)
        row = FaceVerification.of_gallery(gal).compute(far=(a.far,))["at_far"][0]
        res = bench(gal.rows, labels, row["threshold"], a.min_samples, a.iters)
        print(json.dumps({"set": "planted", "N": N, "D": D, "identities": a.identities, "far": a.far,
                          "threshold": row["threshold"], "tar": row["tar"], "min_samples": a.min_samples, **res}),
              flush=True)
        one = FaceGallery(dim=D, capacity=N, device=dev)
        one.add(torch.randn(1, D, device=dev, generator=gen) + 0.1 * torch.randn(N, D, device=dev, generator=gen),
                [0] * N)
        worst = bench(one.rows, torch.zeros(N, device=dev, dtype=torch.int64), row["threshold"], a.min_samples,
                      a.iters)
        assert worst["clusters"] == 1 and worst["edges"] == N * (N - 1) // 2
        print(json.dumps({"set": "one identity", "N": N, "D": D, "threshold": row["threshold"],
                          "min_samples": a.min_samples, **worst,
                          "link_over_planted_link": round(worst["link"]["ms"] / res["link"]["ms"], 3)}), flush=True)
        del gal, one
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
