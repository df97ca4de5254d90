"""Time the NV12 routes (csrc/nv12.hip) against conversion followed by the uint8 kernels, on the
same machine in the same run.

    python tools/nv12_bench.py [--iters 20] [--scale 1.0]

256 frames of 1080 x 1920 NV12 on decoder-like surfaces (pitch 2048, chroma from row 1088):
  case 1, whole-frame ingest into a 640 x 640 letterbox, norm "unit":
    a  convert_ingest : prpe_nv12_to_rgb into a staging tensor, then prpe_frame_ingest on it;
    b  fused_ingest   : prpe_frame_ingest_nv12;
  case 2, 1024 person crops (4 per frame, the box sizes of tools/crop_bench.py placed in the 1080p frame):
    c  convert_crop   : prpe_nv12_to_rgb, then prpe_crop_resize_u8;
    d  fused_crop     : prpe_crop_resize_nv12;
  and prpe_nv12_to_rgb alone (convert).
--scale shrinks the frame COUNT (not the sizes) for a quick look.
HIP-event timing around the ops wrappers, 3 warm-ups per route, the routes alternated inside each
iteration, medians with (min, max). The planes (0.83 GB) and the staging tensor (1.59 GB) are many
times the 256 MiB Infinity Cache, so a replay finds neither in cache: these are HBM figures.
One JSON line per route to stdout and to profiles/nv12_bench.jsonl: ms, the bytes the route must
move at least (for the ingest: the source pixels a 2-tap 3x downscale touches are not counted
apart, the whole planes are), TB/s and its share of the 6.29 TB/s float4 copy, the
share of the 155 ms model step, the staging bytes the route needs, and equal: the fused route has
the unfused route's bits.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd"))

from prpe import FrameIngest, NV12Frames, ops, synth  # noqa: E402

CEILING = 6.29e12      # B/s, float4 copy on the MI355X
STEP_MS = 155.0        # the model step at bs = 256 (README)
HS, WS, PITCH, UV_ROW = 1080, 1920, 2048, 1088
CH, CW = 256, 192


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nv12_bench needs the MI355X"
    dev = "cuda:0"
    B, P = max(1, int(256 * a.scale)), 4
    gen = torch.Generator(device=dev).manual_seed(1)
    surf = torch.randint(0, 256, (B, UV_ROW + HS // 2, PITCH), device=dev, dtype=torch.uint8, generator=gen)
    nv = NV12Frames.from_surface(surf, HS, WS, uv_row=UV_ROW)
    ing = FrameIngest(size=(640, 640), mode="letterbox", norm="unit")
    geom = ing.geometry(HS, WS)
    rgb = torch.empty(B, HS, WS, 3, device=dev, dtype=torch.uint8)          # the staging copy
    bufs = [torch.zeros(B, 646, 648, 4, device=dev) for _ in range(2)]
    ya, yb = (b[:, 3:643, 3:643, :] for b in bufs)

    # case 2's list: crop_bench's box sizes, placed inside the 1080p frame
    n = B * P
    box = synth.uniform(3, "crop_bench:boxes", (B, P, 4))
    w, h = 60 + 140 * box[..., 2], 150 + 300 * box[..., 3]
    x1, y1 = box[..., 0] * (WS - w), box[..., 1] * (HS - h)
    score = torch.linspace(0.9, 0.5, P).expand(B, P)
    dets = torch.stack([x1, y1, x1 + w, y1 + h, score, torch.zeros(B, P)], 2).to(dev)
    counts = torch.full((B,), P, device=dev, dtype=torch.int32)
    meta = torch.empty(n, 8, device=dev)
    n_crops = torch.empty(1, device=dev, dtype=torch.int32)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    ops.crop_select(dets, counts, (HS, WS), crop_meta=meta, n_crops=n_crops, status=status, max_per_frame=P)
    assert int(n_crops) == n and int(status) == 0
    crops = [torch.zeros(n, CH + 4, CW + 4, 4, device=dev) for _ in range(2)]

    def convert_ingest():
        ops.nv12_to_rgb(nv, rgb)
        ops.frame_ingest(rgb, ya, geom, ing.a, ing.b, ing.fill)

    def convert_crop():
        ops.nv12_to_rgb(nv, rgb)
        ops.crop_resize_u8(rgb, meta, n_crops, crops[0], ing.a, ing.b)

    routes = {"convert": lambda: ops.nv12_to_rgb(nv, rgb),
              "a_convert_ingest": convert_ingest,
              "b_fused_ingest": lambda: ops.frame_ingest_nv12(nv, yb, geom, ing.a, ing.b, ing.fill),
              "c_convert_crop": convert_crop,
              "d_fused_crop": lambda: ops.crop_resize_nv12(nv, meta, n_crops, crops[1], ing.a, ing.b)}
    for f in routes.values():
        f()
    torch.cuda.synchronize()
    equal = {"b_fused_ingest": bool(torch.equal(bufs[0].view(torch.int32), bufs[1].view(torch.int32))),
             "d_fused_crop": bool(torch.equal(crops[0].view(torch.int32), crops[1].view(torch.int32)))}
    t = timed(routes, a.iters)

    planes = B * (HS * WS + (HS // 2) * WS)                   # what a route reads of the surfaces at most
    staging = rgb.numel()
    stem, crop_out = B * 640 * 640 * 16, n * CH * CW * 16
    # bytes each route moves at least: conversion reads the planes and writes the staging copy; the
    # unfused routes then read (at most) that copy again; every route writes its 16 B per output pixel
    moved = {"convert": planes + staging, "a_convert_ingest": planes + 2 * staging + stem,
             "b_fused_ingest": planes + stem, "c_convert_crop": planes + staging + crop_out,
             "d_fused_crop": crop_out}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "nv12_bench.jsonl"), "w") as fh:
        for k, (ms, lo, hi) in t.items():
            fused = k in ("b_fused_ingest", "d_fused_crop")
            out = {"route": k, "frames": B, "crops": n if "crop" in k else 0, "ms": round(ms, 4), "min": round(lo, 4),
                   "max": round(hi, 4), "bytes": moved[k], "TBps": round(moved[k] / ms / 1e9, 3),
                   "share": round(moved[k] / (ms * 1e-3) / CEILING, 3), "floor_ms": round(moved[k] / CEILING * 1e3, 4),
                   "step_share": round(ms / STEP_MS, 5), "staging_bytes": 0 if fused else staging}
            if fused:
                out["equal"] = equal[k]
            line = json.dumps(out)
            print(line, flush=True)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
