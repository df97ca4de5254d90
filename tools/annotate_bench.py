"""Time prpe_annotate_nv12 / prpe_annotate_u8 against their floor, their ceiling and the host route
they replace.

    python tools/annotate_bench.py [--frames 256] [--per-frame 8] [--iters 20] [--host-frames 1]

Workload: ``frames`` frames of 1920 x 1080, ``per-frame`` persons (windows 150 x 400 px, 17
keypoints, the COCO limbs) and as many faces (100 x 100 px, pixelated) per frame, for both twins:
NV12 (one surface per frame, pitch 1920) and packed uint8 RGB.
Routes, alternated inside each iteration after 3 warm-ups, device events, median of ``iters`` with
(min, max):
  paint : ops.annotate_* on the full lists (two launches);
  empty : the same call with n_p = n_f = 0: what the launches cost when no tile is touched;
  copy  : a device-to-device copy of the same surfaces: what a design that passes over the whole
          frame could not beat.
  host  : what a caller of the previous commit has, for ``host-frames`` frames only and SCALED to
          ``frames`` (said so in the output): one read of the surface to the host, the numpy
          restatement of tests/test_annotate_host.py there, one write back; wall-clock.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from prpe import NV12Frames, ops  # noqa: E402

H, W, K = 1080, 1920, 17


def lists(B, P):
    """Person and face lists on the host: numpy arrays as tests/test_annotate_host.case lays them out."""
    g = np.random.default_rng(0)
    n = B * P
    frame = np.repeat(np.arange(B, dtype=np.int32), P)
    x0 = (np.tile(np.arange(P), B) * (W - 200) / max(P, 1) + g.uniform(0, 40, n)).astype(np.float32)
    y0 = g.uniform(100, H - 520, n).astype(np.float32)
    meta_p = np.zeros((n, 8), np.float32)
    meta_p.view(np.int32)[:, 0] = frame
    meta_p[:, 2], meta_p[:, 3], meta_p[:, 4], meta_p[:, 5], meta_p[:, 6] = x0, y0, 150.0, 400.0, 0.9
    kp = np.stack([x0[:, None] + g.uniform(0, 150, (n, K)), y0[:, None] + g.uniform(0, 400, (n, K)),
                   np.full((n, K), 0.9)], 2).astype(np.float32)
    meta_f = meta_p.copy()
    meta_f[:, 2], meta_f[:, 3], meta_f[:, 4], meta_f[:, 5] = x0 + 25.0, y0 - 90.0, 100.0, 100.0
    return dict(meta_p=meta_p, kpts=kp, pcol=(np.arange(n) % 12).astype(np.int32), meta_f=meta_f,
                fmode=np.ones(n, np.int32), fcol=np.zeros(n, np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--per-frame", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "annotate_bench needs the MI355X"
    dev = "cuda:0"
    B, P = a.frames, a.per_frame
    n = B * P
    L = lists(B, P)
    t = {k: torch.from_numpy(v).to(dev) for k, v in L.items()}
    full = torch.tensor([n], dtype=torch.int32, device=dev)
    none = torch.zeros(1, dtype=torch.int32, device=dev)
    palette = torch.randint(0, 256, (13, 4), dtype=torch.uint8, device=dev)
    table, means = ops.annotate_workspaces(n, n, K, len(ops.COCO_LIMBS), dev)
    g = torch.Generator(device=dev).manual_seed(0)
    surface = torch.randint(0, 256, (B, H * 3 // 2, W), dtype=torch.uint8, device=dev, generator=g)
    nv12 = NV12Frames.from_surface(surface, H, W)
    rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    spare = {"nv12": torch.empty_like(surface), "u8": torch.empty_like(rgb)}

    def paint(kind, count):
        call, frames = (ops.annotate_nv12, nv12) if kind == "nv12" else (ops.annotate_u8, rgb)
        call(frames, palette, persons=(t["meta_p"], count, t["kpts"], t["pcol"]),
             faces=(t["meta_f"], count, t["fmode"], t["fcol"]), table=table, means=means)

    routes = {}
    for kind, src in (("nv12", surface), ("u8", rgb)):
        routes[f"{kind}_paint"] = lambda kind=kind: paint(kind, full)
        routes[f"{kind}_empty"] = lambda kind=kind: paint(kind, none)
        routes[f"{kind}_copy"] = lambda kind=kind, src=src: spare[kind].copy_(src)
    for _ in range(3):
        for f in routes.values():
            f()
    times = {k: [] for k in routes}
    for _ in range(a.iters):
        for k, f in routes.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    result = {"frames": B, "persons_per_frame": P, "faces_per_frame": P, "iters": a.iters, "size": [H, W],
              "surface_mb": {"nv12": round(surface.numel() / 1e6, 1), "u8": round(rgb.numel() / 1e6, 1)},
              "ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
              "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}

    # the host route on the first frames, scaled
    import test_annotate_host as AH
    hf = max(1, min(a.host_frames, B))
    c = AH.case(hf, H, W)
    keep = slice(0, hf * P)
    c.update(meta_p=L["meta_p"][keep], n_p=hf * P, kpts=L["kpts"][keep], pcol=L["pcol"][keep], meta_f=L["meta_f"][keep],
             n_f=hf * P, fmode=L["fmode"][keep], fcol=L["fcol"][keep], palette=palette.cpu().numpy())
    host = {}
    for kind in ("nv12", "u8"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "nv12":
            s = surface[:hf].cpu().numpy()                                            # the one read
            y, uv = s[:, :H], s[:, H:].reshape(hf, H // 2, W // 2, 2)
            yo, uvo, _ = AH.annotate_nv12_ref(c, y, uv)
            back = np.concatenate([yo, uvo.reshape(hf, H // 2, W)], 1)
            surface[:hf].copy_(torch.from_numpy(back))                               # the one write
        else:
            out, _ = AH.annotate_u8_ref(c, rgb[:hf].cpu().numpy())
            rgb[:hf].copy_(torch.from_numpy(out))
        torch.cuda.synchronize()
        host[kind] = (time.perf_counter() - t0) * 1e3
    result["host_ms_measured"] = {k: round(v, 1) for k, v in host.items()}
    result["host_frames_measured"] = hf
    result["host_ms_scaled_to_all_frames"] = {k: round(v * B / hf, 1) for k, v in host.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
