"""Time the passes of the on-device identification evaluation (prpe_ident_best, prpe_ident_rank,
prpe_ident_finish) with prpe_pair_hist on the same operands as the yardstick, and against the route
a caller had before them.

    python tools/ident_eval_bench.py [--probes 4096] [--rows 32768] [--iters 20]

D = 512, 1000 identities (a unit-variance centre per identity plus unit-variance noise), two shapes:
  cross : --probes probes (every tenth a stranger to the gallery) against --rows enrolled rows;
  self  : leave-one-out on the --rows enrolled rows.
Routes, all on the same enrolled rows:
  pair_hist : ops.pair_hist, the same tile product with the histogram epilogue (cross / self);
  best, rank, finish : the three stages, each with the zeroing of its outputs;
  parent : blocks of at most 2048 probes: torch.matmul against all rows, the rows that do not take
           part (and, in self mode, the diagonal) set to -inf, the best mate and best non-mate by two
           masked max, and the rank by counting the non-mates above the best mate (ties: lower row
           first). Its [2048, rows] score block and two masked copies are stored.
Both routes must find the same rank-1 probes up to ties the two routes round apart (reported, not
asserted: the parent's matmul has other score bits). HIP-event timing, 3 warm-ups per route, the
routes alternated inside each iteration, medians with (min, max). One JSON line per shape.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from prpe import ops  # noqa: E402
from pair_hist_bench import D, PEAK_TF, timed  # noqa: E402

BLOCK = 2048


def enrolled(x):
    rows, norms = torch.empty_like(x), torch.empty(x.shape[0], device=x.device)
    ops.gallery_enrol(x, rows, norms, 0)
    return rows


def case(name, a, la, b, lb, nbins, iters):
    dev = a.device
    M, N = a.shape[0], (a if b is None else b).shape[0]
    cross = {} if b is None else {"b": b, "b_labels": lb}
    z64 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int64)
    mate, non, skipped, rm1 = z64(M), z64(M), z64(1), torch.zeros(M, device=dev, dtype=torch.int32)
    hist, rank_hist, counts = z64(3, nbins), z64(ops.IDENT_RANKS + 1), z64(4)
    per = {k: torch.empty(M, device=dev, dtype=t) for k, t in (("mate_score", torch.float32), ("non_score", torch.float32),
                                                              ("mate_row", torch.int32), ("non_row", torch.int32),
                                                              ("rank", torch.int32))}
    ph, ps = z64(2, nbins), z64(1)
    got = {}

    def pair_hist():
        ph.zero_()
        ps.zero_()
        ops.pair_hist(a, la, b, lb, nbins=nbins, hist=ph, skipped=ps)

    def best():
        mate.zero_()
        non.zero_()
        skipped.zero_()
        ops.ident_best(a, la, mate_key=mate, non_key=non, skipped=skipped, **cross)

    def rank():
        rm1.zero_()
        ops.ident_rank(a, la, mate_key=mate, rank_minus_1=rm1, **cross)

    def finish():
        hist.zero_()
        rank_hist.zero_()
        counts.zero_()
        ops.ident_finish(la, mate_key=mate, non_key=non, rank_minus_1=rm1, nbins=nbins, hist=hist, rank_hist=rank_hist,
                         counts=counts, **per)

    def parent():
        rows_b, labels_b = (a, la) if b is None else (b, lb)
        ranks = torch.zeros(M, device=dev, dtype=torch.int64)
        cols = torch.arange(N, device=dev)[None, :]
        for r0 in range(0, M, BLOCK):
            r1 = min(r0 + BLOCK, M)
            s = torch.matmul(a[r0:r1], rows_b.t())
            if b is None:
                s[torch.arange(r1 - r0, device=dev), torch.arange(r0, r1, device=dev)] = float("-inf")
            same = la[r0:r1, None] == labels_b[None, :]
            ms, mrow = torch.where(same, s, float("-inf")).max(dim=1)
            nonm = torch.where(same, float("-inf"), s)
            ahead = (nonm > ms[:, None]) | ((nonm == ms[:, None]) & (cols < mrow[:, None]))
            ranks[r0:r1] = torch.where(torch.isfinite(ms), ahead.sum(dim=1) + 1, 0)
        got["rank"] = ranks

    t = timed({"pair_hist": pair_hist, "best": best, "rank": rank, "finish": finish, "parent": parent}, iters)
    torch.cuda.synchronize()
    tiles_m, tiles_n = -(-M // ops.PAIR_HIST_TILE), -(-N // ops.PAIR_HIST_TILE)
    ntiles = tiles_m * (tiles_m + 1) // 2 if b is None else tiles_m * tiles_n
    flop = 2.0 * ntiles * ops.PAIR_HIST_TILE ** 2 * D
    fused = t["best"]["ms"] + t["rank"]["ms"] + t["finish"]["ms"]
    c = counts.cpu().tolist()
    out = {"shape": name, "M": M, "N": N, "D": D, "nbins": nbins, **t,
           "best_over_pair_hist": round(t["best"]["ms"] / t["pair_hist"]["ms"], 3),
           "rank_over_pair_hist": round(t["rank"]["ms"] / t["pair_hist"]["ms"], 3),
           "three_stages_ms": round(fused, 4), "speedup_over_parent": round(t["parent"]["ms"] / fused, 2),
           "best_exec_TFps": round(flop / t["best"]["ms"] / 1e9, 2),
           "best_share_of_peak": round(flop / t["best"]["ms"] / 1e9 / PEAK_TF, 3),
           "mated": c[0], "non_mated": c[1], "rank1": int(rank_hist[0]), "skipped": int(skipped),
           "ranks_differing_from_parent": int((per["rank"].long() != got["rank"]).sum()),
           "parent_score_block_bytes": min(BLOCK, M) * N * 4}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--nbins", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--identities", type=int, default=1000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ident_eval_bench needs the MI355X"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    centres = torch.randn(a.identities + a.identities // 10, D, device=dev, generator=gen)

    def rows_of(n, identities):
        labels = torch.randint(0, identities, (n,), device=dev, generator=gen)
        return enrolled(centres[labels] + torch.randn(n, D, device=dev, generator=gen)), labels

    gallery, lg = rows_of(a.rows, a.identities)
    probes, lp = rows_of(a.probes, centres.shape[0])               # labels past --identities: strangers
    case("cross", probes, lp, gallery, lg, a.nbins, a.iters)
    case("self", gallery, lg, None, None, a.nbins, a.iters)


if __name__ == "__main__":
    main()
