"""Time prpe_crop_resize against the torch route it replaces.

    python tools/crop_bench.py [--frames 256] [--per-frame 4] [--iters 30]

Both routes fill the same zero-bordered NHWC4 crop buffer from the same crop list
(frames [B,3,640,640], per-frame person-like boxes through prpe_crop_select):
  kernel : ops.crop_resize, one launch;
  torch  : ONE F.grid_sample over all frames (the per_frame crops of a frame stacked along the
           output height, so no frame is copied) + per_frame ops.copy_pad launches into the
           buffer, with the sampling grid prebuilt ("torch") or rebuilt by F.affine_grid every
           call ("torch+grid").
HIP-event timing, every route warmed, the routes alternated inside each iteration, medians.
Prints one JSON line; also checks the two routes agree to fp32 resampling accuracy.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd"))

from prpe import ops, synth  # noqa: E402

CH, CW = 256, 192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--per-frame", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "crop_bench needs the MI355X"
    dev = "cuda:0"
    B, P, H, W = a.frames, a.per_frame, 640, 640
    n = B * P
    frames = torch.rand(B, 3, H, W, device=dev)
    box = synth.uniform(3, "crop_bench:boxes", (B, P, 4))
    w, h = 60 + 140 * box[..., 2], 150 + 300 * box[..., 3]
    x1, y1 = box[..., 0] * (W - w), box[..., 1] * (H - h)
    score = torch.linspace(0.9, 0.5, P).expand(B, P)
    dets = torch.stack([x1, y1, x1 + w, y1 + h, score, torch.zeros(B, P)], 2).to(dev)
    counts = torch.full((B,), P, device=dev, dtype=torch.int32)
    meta = torch.empty(n, 8, device=dev)
    n_crops = torch.empty(1, device=dev, dtype=torch.int32)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    ops.crop_select(dets, counts, (H, W), crop_meta=meta, n_crops=n_crops, status=status, max_per_frame=P)
    assert int(n_crops) == n and int(status) == 0
    buf_k = torch.zeros(n, CH + 4, CW + 4, 4, device=dev)
    buf_t = torch.zeros_like(buf_k)

    def theta():
        x0, y0, ww, hh = (meta[:, c] for c in (2, 3, 4, 5))
        z = torch.zeros_like(x0)
        return torch.stack([torch.stack([ww / W, z, (2 * x0 + ww) / W - 1], 1),
                            torch.stack([z, hh / H, (2 * y0 + hh) / H - 1], 1)], 1)

    def make_grid():
        # [n, CH, CW, 2] -> the P crops of a frame stacked along the output height
        return F.affine_grid(theta(), (n, 3, CH, CW), align_corners=False).view(B, P * CH, CW, 2)

    grid = make_grid()

    def torch_route(g):
        out = F.grid_sample(frames, g, mode="bilinear", padding_mode="zeros", align_corners=False)
        out = out.view(B, 3, P, CH, CW)
        slots = buf_t.view(B, P, CH + 4, CW + 4, 4)
        for k in range(P):
            ops.copy_pad(out[:, :, k].permute(0, 2, 3, 1), slots[:, k, 2:2 + CH, 2:2 + CW, :])

    routes = {"kernel": lambda: ops.crop_resize(frames, meta, n_crops, buf_k),
              "torch": lambda: torch_route(grid),
              "torch+grid": lambda: torch_route(make_grid())}
    for f in routes.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    diff = float((buf_k - buf_t).abs().max())
    times = {k: [] for k in routes}
    for _ in range(a.iters):
        for k, f in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    written = n * CH * CW * 16
    print(json.dumps({"crops": n, "frames": [B, 3, H, W], "iters": a.iters,
                      "ms": {k: round(v, 4) for k, v in med.items()},
                      "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                      "kernel_written_GBps": round(written / med["kernel"] / 1e6, 1),
                      "max_abs_diff_kernel_vs_torch": diff}))
    # torch's device grid_sample forms pixel coordinates in fp32: near 640 one ulp is 6e-5 of a
    # pixel, and a few of them times a gradient of up to 1 per pixel is what separates the routes
    assert diff < 1e-3, diff


if __name__ == "__main__":
    main()
