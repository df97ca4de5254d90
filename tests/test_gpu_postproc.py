"""GPU: NMS and soft-argmax kernels against the reference's own outputs (golden vectors made
by the reference code, oracle/make_golden.py) and the oracle, incl. edge cases.

Bar: NMS bit-exact (indices/rows/counts) on identical inputs; soft-argmax coords within
1e-6 abs, scores 1e-6 rel, hard-argmax index exact. Soft-argmax is also checked against an fp64
restatement of the oracle at the sizes where its two 256-thread passes change shape (HW below, at
and above 256, W = 1, H = 1, a map larger than the model's) on ties, plateaus, -inf entries, large
magnitudes and the box-scale clamps.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from oracle import model_ref as R
from prpe import ops
from prpe.postproc import keypoints_from_heatmaps, non_max_suppression, non_max_suppression_padded

pytestmark = pytest.mark.gpu


def _load(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _rows_sorted(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


@pytest.mark.parametrize("case", ["det", "evalstep", "stress"])
def test_nms_matches_reference_golden(case):
    g = _load("golden_nms.npz")
    inp = torch.from_numpy(g[f"{case}_in"]).cuda()
    out, cnt = non_max_suppression_padded(inp)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cnt.cpu().numpy(), g[f"{case}_count"])
    got = out.cpu().numpy()
    for i, n in enumerate(g[f"{case}_count"]):
        a, b = got[i, :n], g[f"{case}_out"][i, :n]
        if case == "evalstep":    # multi-label path, tie order unspecified upstream
            a, b = _rows_sorted(a), _rows_sorted(b)
        np.testing.assert_array_equal(a, b)
        assert np.all(got[i, n:] == 0)


@pytest.mark.parametrize("nc,N,frac,B", [(80, 8400, 0.05, 2), (80, 8400, 0.002, 1), (1, 20000, 1.0, 2)])
def test_nms_global_path_many_candidates(nc, N, frac, B):
    """N*nc above the LDS key capacity (16384): the global-workspace path (keys + rocPRIM
    radix sort per image). A raw 80-class YOLO output at A = 8400 (the reference sorts any
    count and keeps <= max_nms = 30000, util.py:126,157): 5 % of the pairs pass conf ->
    33,600 candidates > max_nms, so the truncation is exercised too. Bit-exact vs the oracle."""
    g = torch.Generator().manual_seed(nc * 7 + B)
    cxy = torch.rand(B, 2, N, generator=g) * 600 + 20
    wh = torch.rand(B, 2, N, generator=g) * 80 + 4
    sc = torch.rand(B, nc, N, generator=g)
    sc = torch.where(torch.rand(B, nc, N, generator=g) < frac, sc * 0.99 + 0.01, sc * 0.0009)
    inp = torch.cat([cxy, wh, sc], 1).contiguous()
    out, cnt = non_max_suppression_padded(inp.cuda())
    torch.cuda.synchronize()
    ref = R.non_max_suppression(inp)
    for i in range(B):
        assert cnt[i].item() == len(ref[i])
        np.testing.assert_array_equal(out[i, :cnt[i]].cpu().numpy(), ref[i].numpy())
    assert min(len(r) for r in ref) > 0


def test_host_tensors_are_refused_before_the_abi():
    """A host pointer in a kernel is a GPU memory fault: every wrapper refuses CPU tensors."""
    with pytest.raises(ValueError, match="device tensor"):
        non_max_suppression_padded(torch.rand(1, 5, 20000))
    with pytest.raises(ValueError, match="device tensor"):
        keypoints_from_heatmaps(torch.rand(1, 17, 64, 48))


def test_nms_list_api_and_transposed_layout():
    g = _load("golden_nms.npz")
    inp = torch.from_numpy(g["det_in"]).cuda()
    dets = non_max_suppression(inp)
    out1, cnt1 = ops.nms(inp.transpose(1, 2).contiguous(), 1)      # [B, N, 4+nc] layout
    torch.cuda.synchronize()
    for i, d in enumerate(dets):
        np.testing.assert_array_equal(d.cpu().numpy(), g["det_out"][i, :g["det_count"][i]])
        np.testing.assert_array_equal(out1[i, :cnt1[i]].cpu().numpy(), d.cpu().numpy())


def test_nms_ties_are_stable_by_index():
    # 4 identical boxes, identical scores, far apart classes -> all kept, in index order
    b, n = 1, 6
    x = torch.zeros(b, 5, n)
    x[0, 0] = torch.tensor([10., 10., 10., 100., 200., 300.])
    x[0, 1] = 10.0
    x[0, 2:4] = 4.0
    x[0, 4] = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
    out, cnt = non_max_suppression_padded(x.cuda())
    ref = R.non_max_suppression(x)[0]
    assert int(cnt[0]) == ref.shape[0] == 4
    np.testing.assert_array_equal(out[0, :4].cpu().numpy(), ref.numpy())


def test_nms_empty_and_all_below_threshold():
    x = torch.zeros(3, 5, 50)
    x[:, 2:4] = 5.0
    x[1, 4] = 0.0005                     # below conf 0.001
    x[2, 4, 7] = float("nan")            # NaN never a candidate
    out, cnt = non_max_suppression_padded(x.cuda())
    assert cnt.tolist() == [0, 0, 0]
    assert torch.all(out == 0)


def test_nms_max_det_cap_and_multilabel():
    torch.manual_seed(0)
    x = torch.rand(2, 4 + 3, 400)
    x[:, 0:2] *= 600
    x[:, 2:4] = x[:, 2:4] * 20 + 2
    out, cnt = non_max_suppression_padded(x.cuda())
    ref = R.non_max_suppression(x)
    for i, r in enumerate(ref):
        assert int(cnt[i]) == r.shape[0] == 300
        np.testing.assert_array_equal(out[i, :300].cpu().numpy(), r.numpy())


@pytest.mark.parametrize("case,boxes", [("model", False), ("peaky", True)])
def test_softargmax_matches_reference_golden(case, boxes):
    g = _load("golden_softargmax.npz")
    hm = torch.from_numpy(g[f"{case}_in"]).cuda()
    bx = torch.from_numpy(g["peaky_boxes"]).cuda() if boxes else None
    c, s = keypoints_from_heatmaps(hm, bx)
    torch.cuda.synchronize()
    np.testing.assert_allclose(c.cpu().numpy(), g[f"{case}_coords"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(s.cpu().numpy(), g[f"{case}_scores"], rtol=2e-6, atol=0)


def test_softargmax_hard_argmax_index_exact():
    g = _load("golden_softargmax.npz")
    hm = torch.from_numpy(g["peaky_in"])
    _, _, am = ops.softargmax(hm.cuda(), None, want_argmax=True)
    torch.cuda.synchronize()
    ref = hm.reshape(hm.shape[0], hm.shape[1], -1).argmax(-1).int()
    assert torch.equal(am.cpu(), ref)


# ----------------------------------------------------------------------------- soft-argmax shapes and edges
def _softargmax_ref64(heat, boxes=None):
    """keypoints_from_heatmaps of oracle/model_ref.py restated in fp64 (from the fp32 inputs)."""
    B, K, H, W = heat.shape
    x = heat.double().reshape(B, K, H * W)
    prob = torch.softmax(x, 2)
    idx = torch.arange(H * W)
    xe = (prob * (idx % W).double()).sum(2) + 0.5
    ye = (prob * (idx // W).double()).sum(2) + 0.5
    coords = torch.stack([xe / W, ye / H], -1)
    scores = prob.max(2)[0]
    if boxes is not None:
        b = boxes.double()
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        scores = scores * torch.clamp(torch.sqrt(area) / 96.0, min=0.5, max=2.0).view(-1, 1)
    return coords, scores


def _softargmax_check(heat, boxes=None, first_max=None):
    """Kernel vs fp64: coords 1e-6 abs and scores 2e-6 rel up to the model's 64x48 map; on a larger
    map 4x the fp32 CPU oracle's own error against fp64 on the same input (another summation
    tree), floor 1e-6. The hard-argmax index is exact: the first maximum, as torch.argmax gives."""
    B, K, H, W = heat.shape
    c, s, am = ops.softargmax(heat.cuda(), None if boxes is None else boxes.cuda(), want_argmax=True)
    torch.cuda.synchronize()
    c, s, am = c.cpu(), s.cpu(), am.cpu()
    rc, rs = _softargmax_ref64(heat, boxes)
    atol_c, rtol_s = 1e-6, 2e-6
    if H * W > 64 * 48:
        oc, os_ = R.keypoints_from_heatmaps(heat, boxes)
        atol_c = max(4 * float((oc.double() - rc).abs().max()), 1e-6)
        rtol_s = max(4 * float(((os_.double() - rs).abs() / rs).max()), 1e-6)
    flat = heat.reshape(B, K, H * W)
    ref_am = flat.argmax(-1).int()
    if first_max is not None:
        assert torch.equal(ref_am, first_max.int())
    assert torch.equal(am, ref_am)
    assert torch.isfinite(c).all() and torch.isfinite(s).all()
    np.testing.assert_allclose(c.double().numpy(), rc.numpy(), rtol=0, atol=atol_c)
    np.testing.assert_allclose(s.double().numpy(), rs.numpy(), rtol=rtol_s, atol=0)
    return c, s, am


# HW = 35 (one partial pass of the 256 threads), 256 (exactly one pass), 257 as one row (W > 256),
# 300 as one column (W = 1), the model's 64x48, and 97x33 (odd, 3201 = 12 passes + 129)
SOFTARGMAX_SHAPES = [(2, 3, 5, 7), (1, 2, 16, 16), (1, 2, 1, 257), (2, 1, 300, 1), (2, 17, 64, 48), (1, 3, 97, 33)]


def _heat(kind, shape):
    B, K, H, W = shape
    HW = H * W
    g = torch.Generator().manual_seed(HW * 31 + K + len(kind))
    x = torch.randn(B, K, HW, generator=g) * 3.0
    first = None
    if kind == "constant":
        x[:] = 0.7
    elif kind == "two_maxima":                       # two equal maxima at random places per map
        pos = torch.stack([torch.randperm(HW, generator=g)[:2].sort()[0] for _ in range(B * K)]).view(B, K, 2)
        top = x.max(-1, keepdim=True)[0] + 1.0
        x.scatter_(2, pos, top.expand(B, K, 2))
        first = pos[..., 0]
    elif kind == "max_last":
        x[..., -1] = x.max(-1)[0] + 2.0
        first = torch.full((B, K), HW - 1)
    elif kind == "plateau":                          # 300 equal maxima (half the map where it is smaller)
        n, start = min(300, HW // 2), HW // 7
        x[..., start:start + n] = x.max(-1, keepdim=True)[0] + 1.0
        first = torch.full((B, K), start)
    elif kind == "large":                            # +-1e4: exp(x - max) underflows all but the top
        x = (torch.rand(B, K, HW, generator=g) * 2 - 1) * 1e4
    elif kind == "half_neg_inf":                     # the first half of the map (which holds index 0)
        x[..., :HW // 2] = float("-inf")
    else:
        assert kind == "random"
    return x.reshape(B, K, H, W), first


@pytest.mark.parametrize("kind", ["random", "constant", "two_maxima", "max_last", "plateau", "large", "half_neg_inf"])
@pytest.mark.parametrize("shape", SOFTARGMAX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_softargmax_shapes_and_contents(shape, kind):
    heat, first = _heat(kind, shape)
    c, s, _ = _softargmax_check(heat, first_max=first)
    if kind == "constant":                           # every sum is exact in fp32
        H, W = shape[2:]
        assert torch.equal(c, torch.full_like(c, 0.5))
        np.testing.assert_allclose(s.numpy(), np.full(s.shape, 1.0 / (H * W)), rtol=2e-6, atol=0)
    if kind == "plateau":
        assert int((heat.reshape(*shape[:2], -1) == heat.amax((2, 3)).unsqueeze(-1)).sum(-1).min()) == \
            min(300, shape[2] * shape[3] // 2)


def test_softargmax_box_scale_clamps():
    """score *= clamp(sqrt(area) / 96, 0.5, 2): exactly at, just inside and just outside each clamp,
    zero area (the 0.5 clamp), a non-square box; one box per frame."""
    sides = [(48.0, 48.0), (192.0, 192.0),            # sqrt(area) / 96 exactly 0.5 and exactly 2
             (48.01, 48.01), (47.99, 47.99),          # just inside / outside the lower clamp
             (191.99, 191.99), (192.01, 192.01),      # just inside / outside the upper clamp
             (0.0, 0.0), (0.0, 50.0),                 # zero area
             (24.0, 96.0), (96.0, 96.0), (400.0, 300.0), (3.0, 5.0)]
    B = len(sides)
    x0 = torch.arange(B, dtype=torch.float32) * 7.0 + 3.0
    y0 = torch.arange(B, dtype=torch.float32) * 3.0 + 11.0
    wh = torch.tensor(sides)
    boxes = torch.stack([x0, y0, x0 + wh[:, 0], y0 + wh[:, 1]], 1)
    heat, _ = _heat("random", (B, 2, 5, 7))
    _, s, _ = _softargmax_check(heat, boxes)
    _, s0, _ = _softargmax_check(heat)
    # the exact cases: scale exactly 0.5, 2, 0.5 (zero area), and 1 for the 96x96 box
    for i, f in ((0, 0.5), (1, 2.0), (3, 0.5), (5, 2.0), (6, 0.5), (7, 0.5), (8, 0.5), (9, 1.0), (10, 2.0), (11, 0.5)):
        assert torch.equal(s[i], s0[i] * f), (i, f)
