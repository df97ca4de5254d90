"""Time the wide-batch gallery search (prpe_gallery_topk_wide) against the exact one
(prpe_gallery_topk) on the same machine in the same run.

    python tools/gallery_wide_bench.py [--g 10000 1000000] [--q 16 64 256 2048] [--k 1 5] [--iters 20]
                                       [--exact-lib path/to/the/parent/commit's/libprpe.so]

D = 512, unit-variance random embeddings, every row valid; half the queries are a gallery row plus
noise (a real probe), the rest unrelated.
  exact  : prpe_gallery_topk. With --exact-lib the entry point is taken from that library (a build of
           the parent commit), otherwise from this build (whose exact kernels compile to the same
           code: DESIGN.md §5k, resource table);
  wide   : prpe_gallery_topk_wide of this build;
  forced : prpe_gallery_topk_wide on all-zero queries: every score ties at 0, no query can be
           certified, so every query takes the filter AND the exact fallback (the worst case).
HIP-event timing, 3 warm-ups per route, the routes alternated inside each iteration, medians with
(min, max). One JSON line per case as it finishes. bytes = what the wide route must move at least
(the gallery once, the lists twice, the queries); bf16_flop = the executed bf16-MFMA FLOP of the
filter (queries padded to the 64-wide block); fallback_share = the share of queries with route 1;
equal = the wide outputs have the exact route's bits. wins = the wide route's slowest run is faster
than the exact route's fastest.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd"))

from prpe import ops  # noqa: E402
from prpe._lib import SIGNATURES, lib  # noqa: E402

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


def exact_entry(path):
    """(workspace_bytes, topk) of the exact route: this build's, or those of the library at ``path``."""
    L = lib()
    if path:
        L = C.CDLL(path)
        for name in ("prpe_gallery_topk_workspace_bytes", "prpe_gallery_topk"):
            getattr(L, name).restype, getattr(L, name).argtypes = SIGNATURES[name]
    return L.prpe_gallery_topk_workspace_bytes, L.prpe_gallery_topk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, nargs="+", default=[10_000, 1_000_000])
    ap.add_argument("--q", type=int, nargs="+", default=[16, 64, 256, 2048])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--exact-lib", default=None, help="a libprpe.so built from the parent commit")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gallery_wide_bench needs the MI355X"
    dev = "cuda:0"
    exact_bytes, exact_topk = exact_entry(a.exact_lib)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(1)
    for G in a.g:
        x = torch.randn(G, D, device=dev, generator=gen)
        gal, norms = torch.empty(G, D, device=dev), torch.empty(G, device=dev)
        ops.gallery_enrol(x, gal, norms, 0)
        del x
        for Q in a.q:
            q = torch.randn(Q, D, device=dev, generator=gen)
            q[: (Q + 1) // 2] = gal[: (Q + 1) // 2] + 0.3 * q[: (Q + 1) // 2] / D ** 0.5
            zeros = torch.zeros_like(q)
            for k in a.k:
                es, er = torch.empty(Q, k, device=dev), torch.empty(Q, k, device=dev, dtype=torch.int32)
                ws_, wr = torch.empty_like(es), torch.empty_like(er)
                fs, fr = torch.empty_like(es), torch.empty_like(er)
                route, froute = (torch.empty(Q, device=dev, dtype=torch.uint8) for _ in range(2))
                ews = torch.empty(exact_bytes(Q, G, k), device=dev, dtype=torch.uint8)
                wws = torch.empty(lib().prpe_gallery_topk_wide_workspace_bytes(Q, G, k), device=dev, dtype=torch.uint8)

                def exact():
                    rc = exact_topk(q.data_ptr(), D, Q, D, gal.data_ptr(), G, None, k, es.data_ptr(), er.data_ptr(), None,
                                    0.0, None, ews.data_ptr(), ews.numel(), stream())
                    assert rc == 0, rc

                routes = {
                    "exact": exact,
                    "wide": lambda: ops.gallery_topk_wide(q, gal, G, k, scores=ws_, rows=wr, route=route, workspace=wws),
                    "forced": lambda: ops.gallery_topk_wide(zeros, gal, G, k, scores=fs, rows=fr, route=froute,
                                                            workspace=wws),
                }
                t = timed(routes, a.iters)
                torch.cuda.synchronize()
                nqb, chunk, nchunks = ops.gallery_wide_plan(Q, G)
                moved = G * D * 4 + 2 * nchunks * Q * (ops.GALLERY_WIDE_L * 8 + 4) + Q * D * 10
                flop = 2.0 * nqb * ops.GALLERY_WIDE_QB * G * D
                out = {"Q": Q, "G": G, "D": D, "k": k, "plan": [nqb, chunk, nchunks], **t, "bytes": moved,
                       "bf16_flop": flop, "wide_TBps": round(moved / t["wide"]["ms"] / 1e9, 3),
                       "gallery_reads": nqb, "wide_reread_TBps": round(nqb * G * D * 4 / t["wide"]["ms"] / 1e9, 3),
                       "wide_bf16_TFps": round(flop / t["wide"]["ms"] / 1e9, 2),
                       "fallback_share": float(route.float().mean()),
                       "forced_fallback_share": float(froute.float().mean()),
                       "equal": bool(torch.equal(ws_.view(torch.int32), es.view(torch.int32)) and torch.equal(wr, er)),
                       "speedup": round(t["exact"]["ms"] / t["wide"]["ms"], 3),
                       "wins": t["wide"]["max"] < t["exact"]["min"],
                       "exact_from": a.exact_lib or "this build"}
                print(json.dumps(out), flush=True)
        del gal
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
