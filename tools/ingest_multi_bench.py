"""Time the mixed-size / antialiased ingest (prpe_frame_ingest_multi) against prpe_frame_ingest on
the same machine in the same run.

    python tools/ingest_multi_bench.py [--iters 20] [--scale 1.0]

Every case letterboxes into 640 x 640 (the stem's buffer [B, 646, 648, 4]), norm "unit":
  a  single     : prpe_frame_ingest,             256 frames of 1080 x 1920 (one tensor);
  b  multi_bil  : prpe_frame_ingest_multi, filter 0, the same frames (8 launches of 32);
  c  multi_aa   : prpe_frame_ingest_multi, filter 1, the same frames;
  d  aa_4k      : filter 1, 64 frames of 2160 x 3840;
  e  aa_mixed   : filter 1, 96 x 720p + 96 x 1080p + 64 x 4K in one batch, interleaved.
--scale shrinks the frame COUNTS (not the sizes) for a quick look.
HIP-event timing of the library calls (the table of frames built once), 3 warm-ups per route, a/b/c
alternated inside each iteration, medians with (min, max). Cache state: every case's source (0.9-1.6 GB) plus its destination (0.4-1.7 GB) is several
times the 256 MiB Infinity Cache, so a replay finds neither in cache: the figures are HBM figures.
One JSON line per case: ms, the source bytes, src_TBps = source bytes / time and its share of the
6.29 TB/s the project measured for a float4 copy, all_TBps = (source + the 16 B stored
per model pixel) / time and its share -- the kernel cannot be faster than the second -- and the
step's share against the 155 ms model step. equal: b has a's bits.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd"))

from prpe import FrameIngest, ops  # noqa: E402
from prpe._lib import IngestSrc, lib  # noqa: E402

CEILING = 6.29e12      # B/s, float4 copy on the MI355X
STEP_MS = 155.0        # the model step at bs = 256 (README)
SIZES = {"720p": (720, 1280), "1080p": (1080, 1920), "4k": (2160, 3840)}


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
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def report(name, frames, t, extra=None):
    ms, lo, hi = t
    src = sum(f.shape[0] * f.shape[1] * 3 for f in frames)
    stored = len(frames) * 640 * 640 * 16
    out = {"case": name, "frames": len(frames), "ms": round(ms, 4), "min": round(lo, 4), "max": round(hi, 4),
           "src_bytes": src, "src_TBps": round(src / ms / 1e9, 3), "src_share": round(src / (ms * 1e-3) / CEILING, 3),
           "all_TBps": round((src + stored) / ms / 1e9, 3),
           "all_share": round((src + stored) / (ms * 1e-3) / CEILING, 3),
           "floor_ms_src": round(src / CEILING * 1e3, 4), "floor_ms_all": round((src + stored) / CEILING * 1e3, 4),
           "step_share": round(ms / STEP_MS, 5), **(extra or {})}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_multi_bench needs the MI355X"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    cnt = lambda n: max(1, int(n * a.scale))
    ing = FrameIngest(size=(640, 640), mode="letterbox", norm="unit")
    rand = lambda n, hw: torch.randint(0, 256, (n, *hw, 3), device=dev, dtype=torch.uint8, generator=gen)

    def dest(B):
        buf = torch.zeros(B, 646, 648, 4, device=dev)
        return buf, buf[:, 3:643, 3:643, :]

    def multi(frames, y, filt):
        """The library call on a table built once: what is timed is the device, not Python's loop
        over the frames (wrapper_host_ms reports that loop, ops.frame_ingest_multi, on its own)."""
        geoms = ing.geometry_batch([f.shape[:2] for f in frames]).tolist()
        table = (IngestSrc * len(frames))(*[IngestSrc(f.data_ptr(), f.shape[0], f.shape[1], *f.stride(), *g)
                                            for f, g in zip(frames, geoms)])
        yv, f3 = ops.view(y), [(C.c_float * 3)(*v) for v in (ing.a, ing.b, ing.fill)]

        def call():
            rc = lib().prpe_frame_ingest_multi(table, len(frames), C.byref(yv), filt, *f3, int(ing.swap_rb), None,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
        return call

    def wrapper_host_ms(frames, y, filt):
        geoms = ing.geometry_batch([f.shape[:2] for f in frames])
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.frame_ingest_multi(frames, y, geoms, filt, ing.a, ing.b, ing.fill, ing.swap_rb)
            ts.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        return round(statistics.median(ts), 4)

    # a, b, c: 256 x 1080p
    B = cnt(256)
    u8 = rand(B, SIZES["1080p"])
    frames = list(u8.unbind(0))
    (buf_a, ya), (buf_b, yb) = dest(B), dest(B)
    geom = ing.geometry(*SIZES["1080p"])
    routes = {"single": lambda: ops.frame_ingest(u8, ya, geom, ing.a, ing.b, ing.fill, ing.swap_rb),
              "multi_bil": multi(frames, yb, 0), "multi_aa": multi(frames, yb, 1)}
    routes["single"]()
    routes["multi_bil"]()
    torch.cuda.synchronize()
    equal = bool(torch.equal(buf_a.view(torch.int32), buf_b.view(torch.int32)))
    t = timed(routes, a.iters)
    report("a_single_1080p", frames, t["single"])
    report("b_multi_bilinear_1080p", frames, t["multi_bil"],
           {"equal": equal, "vs_single_ms": round(t["multi_bil"][0] - t["single"][0], 4), "launches": -(-B // 32),
            "wrapper_host_ms": wrapper_host_ms(frames, yb, 0)})
    report("c_multi_antialias_1080p", frames, t["multi_aa"])
    del u8, frames, buf_a, ya, routes
    torch.cuda.empty_cache()

    # d: 64 x 4K
    B4 = cnt(64)
    u4 = rand(B4, SIZES["4k"])
    f4 = list(u4.unbind(0))
    report("d_antialias_4k", f4, timed({"aa": multi(f4, yb[:B4], 1)}, a.iters)["aa"])

    # e: mixed, interleaved so that every launch of 32 holds all three sizes
    n7, n10, n4 = cnt(96), cnt(96), min(B4, cnt(64))
    u7, u10 = rand(n7, SIZES["720p"]), rand(n10, SIZES["1080p"])
    pools = [list(u7.unbind(0)), list(u10.unbind(0)), f4[:n4]]
    mixed = []
    while any(pools):
        for p in pools:
            if p:
                mixed.append(p.pop())
    _, ym = dest(len(mixed)) if len(mixed) > yb.shape[0] else (None, yb[:len(mixed)])
    report("e_antialias_mixed", mixed, timed({"aa": multi(mixed, ym, 1)}, a.iters)["aa"],
           {"mix": {"720p": n7, "1080p": n10, "4k": n4}})


if __name__ == "__main__":
    main()
