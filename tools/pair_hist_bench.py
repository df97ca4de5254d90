"""Time the fused all-pairs score histogram (prpe_pair_hist) against the route a caller had before
it.

    python tools/pair_hist_bench.py [--n 4096 32768] [--nbins 2048] [--iters 20]

D = 512, 1000 identities (a unit-variance centre per identity plus unit-variance noise), self mode:
the N (N - 1) / 2 pairs of one enrolled set.
  fused  : ops.pair_hist on the enrolled rows; the scores are never stored;
  parent : on the same enrolled rows, torch.matmul of row blocks of at most 4096 rows against the
           rows from the block's first on (the upper part only), the stated bin rule and a
           torch.bincount per block, summed into one histogram. Its [4096, N] score block is stored.
Both routes must count the same genuine and impostor pairs (checked; single bins may differ where
the two routes round a score to different sides of an edge).
HIP-event timing, 3 warm-ups per route, the routes alternated inside each iteration, medians with
(min, max). One JSON line per case. exec_TFps = the executed fp32-MFMA FLOP of the fused route (the
upper triangle of 128 x 128 tiles, 2 T^2 D each) / median; share = of the 157 TF/s fp32 matrix peak.
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

D = 512
PEAK_TF = 157.0
BLOCK = 4096


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
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--nbins", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--identities", type=int, default=1000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pair_hist_bench needs the MI355X"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    nbins, h = a.nbins, a.nbins // 2
    for N in a.n:
        labels = torch.randint(0, a.identities, (N,), device=dev, generator=gen)
        x = torch.randn(a.identities, D, device=dev, generator=gen)[labels] + torch.randn(N, D, device=dev, generator=gen)
        rows, norms = torch.empty(N, D, device=dev), torch.empty(N, device=dev)
        ops.gallery_enrol(x, rows, norms, 0)
        del x
        hist = torch.zeros(2, nbins, device=dev, dtype=torch.int64)
        skipped = torch.zeros(1, device=dev, dtype=torch.int64)
        got = {}

        def fused():
            hist.zero_()
            skipped.zero_()
            ops.pair_hist(rows, labels, nbins=nbins, hist=hist, skipped=skipped)

        def parent():
            out = torch.zeros(2 * nbins, device=dev, dtype=torch.int64)
            for r0 in range(0, N, BLOCK):
                r1 = min(r0 + BLOCK, N)
                s = torch.matmul(rows[r0:r1], rows[r0:].t())
                i = torch.arange(r0, r1, device=dev)[:, None]
                j = torch.arange(r0, N, device=dev)[None, :]
                b = (torch.floor(s * h).clamp_(-h, h - 1).to(torch.int64) + h)
                b += (labels[r0:r1, None] != labels[None, r0:]) * nbins
                out += torch.bincount(b[(i < j) & torch.isfinite(s)], minlength=2 * nbins)
            got["hist"] = out.view(2, nbins)

        t = timed({"fused": fused, "parent": parent}, a.iters)
        torch.cuda.synchronize()
        tiles = -(-N // ops.PAIR_HIST_TILE)
        flop = 2.0 * (tiles * (tiles + 1) // 2) * ops.PAIR_HIST_TILE ** 2 * D
        tf = flop / t["fused"]["ms"] / 1e9
        fh, ph = hist.cpu(), got["hist"].cpu()
        totals = [int(v) for v in fh.sum(dim=1)]
        assert totals == [int(v) for v in ph.sum(dim=1)], (totals, ph.sum(dim=1))
        assert sum(totals) + int(skipped) == N * (N - 1) // 2
        print(json.dumps({"N": N, "D": D, "nbins": nbins, "identities": a.identities, **t,
                          "speedup": round(t["parent"]["ms"] / t["fused"]["ms"], 2),
                          "pairs": N * (N - 1) // 2, "genuine": totals[0], "impostor": totals[1],
                          "fused_exec_TFps": round(tf, 2), "fused_share_of_peak": round(tf / PEAK_TF, 3),
                          "useful_TFps": round(2.0 * (N * (N - 1) // 2) * D / t["fused"]["ms"] / 1e9, 2),
                          "bins_differing_from_parent": int((fh != ph).sum()),
                          "parent_score_block_bytes": min(BLOCK, N) * N * 4}), flush=True)
        del rows, norms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
