"""Micro-benchmark of prpe_attention (ViTPose-B: 192 tokens, 12 heads, d 64) at bs frames (GPU box).

    python tools/attn_bench.py [--batch 256] [--iters 10]

Prints ms per call, executed MFMA TF/s (3 split passes) and the K/V/Q/O bytes moved.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "person-recognition-for-pose-estimation_amd")]

import torch  # noqa: E402

from prpe import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    B, L, H, D = a.batch, 192, 12, 64
    qkv = torch.rand(B * L, 3 * H * D, device="cuda") - 0.5
    out = torch.empty(B * L, H * D, device="cuda")
    ops.attention(qkv, out, B, L, H, D, D ** -0.5)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        ops.attention(qkv, out, B, L, H, D, D ** -0.5)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    fl = 4.0 * B * H * L * L * D
    by = 4.0 * B * L * H * D * 4
    q, k, v = qkv[: 4 * L].view(4, L, 3, H, D).permute(2, 0, 3, 1, 4).double().cpu()
    ref = (torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1) @ v).transpose(1, 2).reshape(4 * L, H * D)
    err = float((out[: 4 * L].double().cpu() - ref).abs().max())
    print(f"max|err| {err:.2e}  attention bs={B}: {ms:.3f} ms  alg {fl / ms / 1e9:.1f} TF/s  exec {3 * fl / ms / 1e9:.1f} TF/s  "
          f"{by / ms / 1e6:.0f} GB/s (q,k,v read + o write)")


def head_major(B=256, iters=10):
    L, H, D = 192, 12, 64
    qkv = torch.rand(B * L, 3 * H * D, device="cuda") - 0.5
    hm = qkv.view(B, L, 3, H, D).permute(0, 2, 3, 1, 4).contiguous()
    del qkv
    st = (3 * H * L * D, H * L * D, L * D, D)
    out = torch.empty(B * L, H * D, device="cuda")
    ops.attention_strided(hm, st, out, B, L, H, D, D ** -0.5)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.attention_strided(hm, st, out, B, L, H, D, D ** -0.5)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    print(f"head-major operand: attention bs={B}: {ms:.3f} ms  {4.0 * B * L * H * D * 4 / ms / 1e6:.0f} GB/s")


if __name__ == "__main__":
    main()
    head_major()
