"""Time the fused cosine top-k (prpe_gallery_topk) against the route a caller had before it
(DESIGN.md §5d).

    python tools/gallery_bench.py [--g 10000 1000000] [--q 1 16 256] [--k 5] [--iters 20]

D = 512, unit-variance random embeddings, every row valid.
  fused  : ops.gallery_topk on an enrolled gallery (queries normalised inside; the [Q, G] scores are
           never stored);
  parent : FaceRecognitionEval.logits' route over the same rows -- ops.l2norm of the queries,
           ops.conv2d at precision 2 over the host-packed [G, 512] matrix into a [Q, G] logits
           tensor -- followed by torch.topk. The pack (the host round trip an enrolment costs on
           that route) is outside the timing.
HIP-event timing, 3 warm-ups per route, the routes alternated inside each iteration, medians with
(min, max). One JSON line per case as it finishes. bytes = G * D * 4 + the partial lists + Q * D * 8
(what the fused kernel must move at least); TBps = bytes / median; exec_TFps = the executed
fp32-MFMA FLOP (queries padded to the 16- or 64-wide block) / median.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd"))

from prpe import ops  # noqa: E402
from prpe._lib import lib  # noqa: E402
from prpe.pack import pack_matrix  # noqa: E402

D = 512


def timed(routes, iters):
    for f in routes.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(iters):
        for k, f in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, nargs="+", default=[10_000, 1_000_000])
    ap.add_argument("--q", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-parent", action="store_true", help="time the fused search only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gallery_bench needs the MI355X"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    for G in a.g:
        x = torch.randn(G, D, device=dev, generator=gen)
        gal, norms = torch.empty(G, D, device=dev), torch.empty(G, device=dev)
        ops.gallery_enrol(x, gal, norms, 0)
        pack = None
        if not a.no_parent:
            pack = pack_matrix("gallery_bench:logits", gal.cpu(), 1, 1, D, 1, 0, dev)
        del x
        for Q in a.q:
            q = torch.randn(Q, D, device=dev, generator=gen)
            q[: (Q + 1) // 2] = gal[: (Q + 1) // 2] + 0.3 * q[: (Q + 1) // 2] / D ** 0.5
            scores = torch.empty(Q, a.k, device=dev)
            rows = torch.empty(Q, a.k, device=dev, dtype=torch.int32)
            nbytes = lib().prpe_gallery_topk_workspace_bytes(Q, G, a.k)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            routes = {"fused": lambda: ops.gallery_topk(q, gal, G, a.k, scores=scores, rows=rows, workspace=ws)}
            got = {}
            if pack is not None:
                qn, qnorm = torch.empty_like(q), torch.empty(Q, device=dev)
                logits = torch.empty(Q, 1, 1, G, device=dev)

                def parent():
                    ops.l2norm(q, qn, qnorm, 1e-12)
                    ops.conv2d(qn.view(Q, 1, 1, D), pack, logits, precision=2)
                    got["s"], got["r"] = torch.topk(logits.view(Q, G), a.k, dim=1)

                routes["parent"] = parent
            t = timed(routes, a.iters)
            torch.cuda.synchronize()
            qb, nqb, chunk, nchunks = ops.gallery_plan(Q, G)
            moved = G * D * 4 + 2 * nchunks * Q * a.k * 8 + Q * D * 8
            flop = 2.0 * nqb * qb * G * D
            out = {"Q": Q, "G": G, "D": D, "k": a.k, "plan": [qb, nqb, chunk, nchunks], **t, "bytes": moved,
                   "fused_TBps": round(moved / t["fused"]["ms"] / 1e9, 3),
                   "fused_exec_TFps": round(flop / t["fused"]["ms"] / 1e9, 2)}
            if pack is not None:
                out["rows_equal_parent"] = bool(torch.equal(rows.long(), got["r"]))
                out["max_abs_score_diff"] = float((scores - got["s"]).abs().max())
                out["parent_logits_bytes"] = Q * G * 4
            print(json.dumps(out), flush=True)
        del gal, pack
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
