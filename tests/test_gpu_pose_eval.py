"""GPU: the pose validation step on device (prpe_pose_eval_loss, prpe_pose_coco_records,
PoseEvalStep) against the REFERENCE's own validation step (tests/golden/golden_pose_eval.npz,
made by tools/make_golden_pose_eval.py) and against the plain-torch restatement of its functions
(tests/test_pose_eval_host.py, pinned there against the same golden on the CPU).

Tolerances (none is taken from what the kernels give):
* target: 4 fp32 ulps of the (b, k) map's peak value per pixel (expf and the fp32 sum's order
  differ from torch's by an ulp or two each); a pixel whose reference value before thresholding
  lies that close to 0.005 may be zero on one side only, and at most 0.1 % of the pixels may
  use that (the fixture has none in the band). Weights exact.
* val_loss: within max(4 e_ref, 16 ulp) of the fp64 restatement's loss, e_ref = |reference fp32
  loss - fp64 loss| (the kernel's reduction tree differs from torch's but is no deeper).
* per-keypoint loss against the fp64 mean of (pred - target)^2 on the kernel's OWN target: the
  kernel accumulates in double and rounds once, so 1 ulp.
* soft-argmax outputs: bit-identical to prpe_softargmax on prpe_flip_average's output.
* records: x, y bit-exact (an FMA contraction would round once where the reference rounds twice),
  v / bbox / area exact, instance score within 16 ulps (a 17-term fp32 sum in another order).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_pose_eval_host as T
from prpe import CombinedModel, PoseEvalStep, ops, synth
from prpe._lib import lib
from prpe.evalsteps import (COCO_FLIP_PAIRS, flip_partner, format_coco_records, joints_mse_keypoint_weights,
                            pose_flip_test)

pytestmark = pytest.mark.gpu
KPW = joints_mse_keypoint_weights()


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.fixture(scope="module")
def gold():
    g = T.load_golden()
    heat, heat_f, batch = T.pose_eval_inputs()
    assert T.inputs_checksum(heat, heat_f, batch) == float(g["input_sum"])
    return g, heat, heat_f, batch


@pytest.fixture(scope="module")
def fused(gold):
    """One fused launch on the golden's inputs, shared by the tests that read its outputs."""
    _, heat, heat_f, batch = gold
    out = ops.pose_eval_loss(heat.cuda(), batch["keypoints"].cuda(), KPW, heat_flipped=heat_f.cuda(),
                             partner=flip_partner(17), mode=0, areas=batch["areas"].cuda(),
                             boxes=batch["boxes"].cuda(), sigma=2.0, topk=8, want_avg=True, want_argmax=True,
                             want_target=True)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_target(got, ref, ref_pre):
    """|got - ref| <= 4 ulp of the map's peak, except band pixels that are zero on one side."""
    tol = T.target_tolerance(ref_pre)
    bad = (got - ref).abs() > tol
    one_sided = (got == 0) != (ref == 0)
    exempt = bad & one_sided & T.band_mask(ref_pre)
    n_exempt = int(exempt.sum())
    print(f"target: max|d| {float((got - ref).abs().max()):.3g}, worst d/tol "
          f"{float(((got - ref).abs() / tol).max()):.3g}, exempt {n_exempt} of {ref.numel()}")
    assert not bool((bad & ~exempt).any())
    assert n_exempt <= T.BAND_CAP * ref.numel()


def test_target_and_weights_vs_golden(gold, fused):
    g, heat, _, batch = gold
    assert np.array_equal(fused["weights"].numpy(), g["weights"])
    pre, _ = T.ref_target(batch["keypoints"], batch["areas"], 64, 48, 2.0, thresholded=False)
    check_target(fused["target"], torch.from_numpy(g["target"]), pre)


def test_val_loss_vs_golden(gold, fused):
    """Measured on the MI355X: e_ref = 1.88e-07 (0.79 ulp of the loss 2.2009745), so the bound is
    16 ulp = 3.8e-06; the fused kernel's distance from the fp64 loss is 5.04e-08 (0.21 ulp)."""
    g = gold[0]
    l64 = float(g["val_loss_fp64"])
    e_ref = abs(float(g["val_loss"]) - l64)
    d = abs(float(fused["loss"][0]) - l64)
    print(f"val_loss: gpu {float(fused['loss'][0]):.9g} fp64 {l64:.12g} e_ref {e_ref:.3g} gpu distance {d:.3g} "
          f"({d / ulp32(l64):.2f} ulp)")
    assert d <= max(4 * e_ref, 16 * ulp32(l64))


def check_loss_chain(out, topk, kpw=KPW):
    """per_kp == the fp64 loss on the kernel's own pred / target / weights rounded once (1 ulp);
    loss == OHKM of per_kp (1 ulp)."""
    B, K = out["avg"].shape[:2]
    mse = ((out["avg"].double() - out["target"].double()).reshape(B, K, -1) ** 2).mean(dim=2)
    ref = mse * out["weights"].double() * torch.as_tensor(kpw, dtype=torch.float32).double().view(1, -1)
    got = out["per_kp"].double()
    assert bool(((got - ref).abs() <= torch.from_numpy(np.spacing(ref.float().abs().numpy())).double()).all())
    B = got.shape[0]
    top = torch.topk(got, topk, dim=1)[0].sum() / (B * topk)
    assert abs(float(out["loss"][0]) - float(top)) <= ulp32(float(top))


def test_per_keypoint_loss_and_ohkm_vs_fp64(fused):
    check_loss_chain(fused, 8)


@pytest.mark.parametrize("mode", ["reference", "swap", "none"])
def test_softargmax_outputs_bit_identical_to_the_unfused_kernels(gold, mode):
    _, heat, heat_f, batch = gold
    h, hf, boxes = heat.cuda(), heat_f.cuda(), batch["boxes"].cuda()
    if mode == "none":
        avg = h
        out = ops.pose_eval_loss(h, batch["keypoints"].cuda(), KPW, boxes=boxes, want_argmax=True)
    else:
        m = 0 if mode == "reference" else 1
        avg = ops.flip_average(h, hf, flip_partner(17), m)
        out = ops.pose_eval_loss(h, batch["keypoints"].cuda(), KPW, heat_flipped=hf, partner=flip_partner(17), mode=m,
                                 boxes=boxes, want_avg=True, want_argmax=True)
        assert torch.equal(out["avg"], avg)
    c, s, am = ops.softargmax(avg, boxes[:, 0], want_argmax=True)
    assert torch.equal(out["coords"], c) and torch.equal(out["scores"], s) and torch.equal(out["argmax"], am)
    c, s = ops.softargmax(avg)
    out = ops.pose_eval_loss(h, batch["keypoints"].cuda(), KPW, heat_flipped=None if mode == "none" else hf,
                             partner=flip_partner(17), mode=1 if mode == "swap" else 0)
    assert torch.equal(out["coords"], c) and torch.equal(out["scores"], s)


# H*W below one wavefront / no multiple of 64, an odd B for the flip(0) mode; 65x65 is past the
# 4096 pixels a workgroup keeps in registers (the re-reading path), in place (avg_out = heat)
@pytest.mark.parametrize("shape,topk,mode,areas", [((3, 2, 17, 10, 7), 2, "reference", True),
                                                   ((1, 1, 5, 3, 5), 2, "swap", False),
                                                   ((2, 3, 4, 65, 65), 2, "reference", False)])
def test_odd_shapes_vs_restatement(shape, topk, mode, areas):
    B, N, K, H, W = shape
    heat, heat_f, kp, ar, boxes = T.random_case(7, *shape)
    ar = ar if areas else None
    pairs = [(a, b) for a, b in COCO_FLIP_PAIRS if b < K]
    part = [-1] * K
    for a, b in pairs:
        part[a], part[b] = b, a
    kpw = [1.0 + 0.25 * k for k in range(K)]
    inplace = H * W > 4096
    h = heat.cuda()
    out = ops.pose_eval_loss(h, kp.cuda(), kpw, heat_flipped=heat_f.cuda(), partner=part,
                             mode=0 if mode == "reference" else 1, areas=None if ar is None else ar.cuda(),
                             boxes=boxes.cuda(), sigma=1.5, topk=topk, avg_out=h if inplace else None,
                             want_avg=True, want_argmax=True, want_target=True)
    out = {k: v.cpu() for k, v in out.items()}
    avg = T.ref_flip_average(heat, heat_f, mode, pairs)
    assert torch.equal(out["avg"], avg)
    target, weights = T.ref_target(kp, ar, H, W, 1.5)
    assert torch.equal(out["weights"], weights)
    if B > 1:
        assert not weights[1].any() and not out["target"][1].any()      # no visible keypoint in the frame
    check_target(out["target"], target, T.ref_target(kp, ar, H, W, 1.5, thresholded=False)[0])
    # loss: the issue's rule with this case's own e_ref, against the fp64 restatement
    t64, w64 = T.ref_target(kp, ar, H, W, 1.5, torch.float64)
    l32 = float(T.ref_loss(avg, target, weights, kpw, topk)[0])
    l64 = float(T.ref_loss(T.ref_flip_average(heat.double(), heat_f.double(), mode, pairs), t64, w64, kpw, topk)[0])
    d = abs(float(out["loss"][0]) - l64)
    print(f"{shape}: loss gpu {float(out['loss'][0]):.9g} fp64 {l64:.12g} e_ref {abs(l32 - l64):.3g} distance {d:.3g}")
    assert d <= max(4 * abs(l32 - l64), 16 * ulp32(l64))
    check_loss_chain(out, topk, kpw)
    # soft-argmax: the unfused kernel on the same average, and the restatement
    c, s, am = ops.softargmax(avg.cuda(), boxes[:, 0].cuda(), want_argmax=True)
    assert torch.equal(out["coords"], c.cpu()) and torch.equal(out["scores"], s.cpu())
    assert torch.equal(out["argmax"], am.cpu())
    rc, rs = T.ref_keypoints(avg, boxes[:, 0])
    torch.testing.assert_close(out["coords"], rc, rtol=0, atol=1e-6)
    torch.testing.assert_close(out["scores"], rs, rtol=1e-5, atol=1e-7)
    assert torch.equal(out["argmax"].long(), avg.reshape(B, K, -1).argmax(dim=2))


def test_deterministic_and_batch_independent(gold):
    _, heat, heat_f, batch = gold
    h, hf, kp, ar, bx = (t.cuda() for t in (heat, heat_f, batch["keypoints"], batch["areas"], batch["boxes"]))

    def run(n, mode):
        return ops.pose_eval_loss(h[:n].contiguous(), kp[:n].contiguous(), KPW, heat_flipped=hf[:n].contiguous(),
                                  partner=flip_partner(17), mode=mode, areas=ar[:n].contiguous(),
                                  boxes=bx[:n].contiguous())
    a, b = run(4, 0), run(4, 0)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["per_kp"], b["per_kp"])
    s4, s2 = run(4, 1), run(2, 1)
    assert torch.equal(s4["per_kp"][:2], s2["per_kp"])
    assert torch.equal(s4["coords"][:2], s2["coords"]) and torch.equal(s4["scores"][:2], s2["scores"])


def _records_on_device(g, batch, keep, cap):
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    kpts = torch.full((cap, 17, 3), -7.0, device="cuda")
    meta = torch.full((cap, 8), -7.0, device="cuda")
    ops.pose_coco_records(torch.from_numpy(g["coords"]).cuda(), torch.from_numpy(g["scores"]).cuda(),
                          batch["boxes"].cuda(), batch["areas"].cuda(), batch["masks"].cuda(),
                          batch["is_crowd"].cuda(), keep, 0.3, 0, counter,
                          kpts, meta)
    torch.cuda.synchronize()
    return int(counter.item()), kpts.cpu().numpy(), meta.cpu().numpy()


def test_records_vs_golden(gold):
    """The reference's coords / scores in, its eval_predictions out: x, y bit for bit."""
    g, _, _, batch = gold
    ref = T.golden_predictions(g)
    n, kpts, meta = _records_on_device(g, batch, [1, 1, 1, 0], 16)
    assert n == len(ref) == 7
    assert (kpts[n:] == -7.0).all() and (meta[n:] == -7.0).all()
    ids = batch["image_ids"]
    preds = format_coco_records(kpts[:n], meta[:n], ids)
    assert meta[:n, 1].copy().view(np.int32).tolist() == [0, 1, 0, 1, 2, 0, 2]     # frame 2's crowd instance 1 skipped
    for p, r in zip(preds, ref):
        assert list(p.keys()) == list(r.keys())
        assert p["image_id"] == r["image_id"] and p["category_id"] == r["category_id"]
        assert p["keypoints"] == r["keypoints"]                        # x, y bit-exact, v exact
        assert p["bbox"] == r["bbox"] and p["area"] == r["area"]
        assert abs(p["score"] - r["score"]) <= 16 * ulp32(r["score"])
    # a second batch appends after the first (frame 3 now kept, the others seen)
    counter = torch.tensor([5], dtype=torch.int64, device="cuda")
    k2 = torch.zeros(16, 17, 3, device="cuda")
    m2 = torch.zeros(16, 8, device="cuda")
    ops.pose_coco_records(torch.from_numpy(g["coords"]).cuda(), torch.from_numpy(g["scores"]).cuda(),
                          batch["boxes"].cuda(), batch["areas"].cuda(), batch["masks"].cuda(),
                          batch["is_crowd"].cuda(), [0, 0, 0, 1], 0.3, 40,
                          counter, k2, m2)
    assert int(counter.item()) == 8
    assert m2[5:8, 0].cpu().numpy().view(np.int32).tolist() == [43, 43, 43] and not m2[:5].any() and not m2[8:].any()


def test_records_overflow_counts_on_and_predictions_raises(gold):
    g, heat, heat_f, batch = gold
    n, kpts, meta = _records_on_device(g, batch, [1, 1, 1, 0], 2)
    assert n == 7                                                       # the true count
    full = _records_on_device(g, batch, [1, 1, 1, 0], 16)
    assert np.array_equal(kpts, full[1][:2]) and np.array_equal(meta, full[2][:2])
    step = PoseEvalStep(None, capacity=2, device="cuda")
    step(batch, heatmaps=heat.cuda(), heatmaps_flipped=heat_f.cuda())
    with pytest.raises(RuntimeError, match="exceed the capacity"):
        step.predictions()


def test_pose_eval_step_on_given_heatmaps_vs_golden(gold, fused):
    g, heat, heat_f, batch = gold
    step = PoseEvalStep(None, device="cuda")
    loss = step(batch, heatmaps=heat.cuda(), heatmaps_flipped=heat_f.cuda())
    assert loss.dim() == 0 and loss.is_cuda and float(loss) == float(fused["loss"][0])
    preds, ref = step.predictions(), T.golden_predictions(g)
    assert len(preds) == len(ref)
    for p, r in zip(preds, ref):
        assert list(p.keys()) == T.PRED_KEYS and p["image_id"] == r["image_id"]
        assert p["keypoints"][2::3] == r["keypoints"][2::3] and p["bbox"] == r["bbox"] and p["area"] == r["area"]
        # coords within 1e-6 of the reference's (prpe_softargmax's bar) times the box extent
        # (<= 220), plus two roundings at |x| < 512 (ulp 3e-5)
        np.testing.assert_allclose(p["keypoints"][0::3], r["keypoints"][0::3], rtol=0, atol=3e-4)
        np.testing.assert_allclose(p["keypoints"][1::3], r["keypoints"][1::3], rtol=0, atol=3e-4)
    # the same batch again: every image id is known, nothing is appended; reset() starts over
    step(batch, heatmaps=heat.cuda(), heatmaps_flipped=heat_f.cuda())
    assert len(step.predictions()) == len(ref)
    step.reset()
    assert step.predictions() == []


def test_records_in_more_than_one_launch_pair():
    """More images than one launch's keep bitmask holds (8192): the next launch pair appends
    after the first, in image order."""
    B, N, K = 8200, 2, 3
    g = torch.Generator().manual_seed(3)
    coords, scores = torch.rand(B, K, 2, generator=g), torch.rand(B, K, generator=g)
    boxes = torch.rand(B, N, 4, generator=g) * 50
    boxes[..., 2:] += boxes[..., :2] + 1
    areas = torch.rand(B, N, generator=g) * 1000
    masks = torch.rand(B, N, generator=g) < 0.7
    crowd = torch.rand(B, N, generator=g) < 0.2
    keep = (torch.rand(B, generator=g) < 0.8).int().tolist()
    keep[8190:8195] = [1, 0, 1, 1, 1]
    masks[8191:8195], crowd[8191:8195] = True, False
    rk, rm = T.ref_records(coords.numpy(), scores.numpy(), boxes, areas, masks, crowd, keep, 0.3, slot_base=5)
    cap = rk.shape[0] + 4
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    kpts, meta = torch.full((cap, K, 3), -7.0, device="cuda"), torch.full((cap, 8), -7.0, device="cuda")
    ops.pose_coco_records(coords.cuda(), scores.cuda(), boxes.cuda(), areas.cuda(), masks.cuda(), crowd.cuda(), keep,
                          0.3, 5, counter, kpts, meta)
    n = int(counter.item())
    assert n == rk.shape[0] and rm[:, 0].copy().view(np.int32).max() > 8192 + 5
    assert np.array_equal(kpts[:n].cpu().numpy(), rk) and bool((kpts[n:] == -7.0).all())
    got = meta[:n].cpu().numpy()
    assert np.array_equal(got[:, :2].view(np.int32), rm[:, :2].view(np.int32)) and np.array_equal(got[:, 3:], rm[:, 3:])
    np.testing.assert_allclose(got[:, 2], rm[:, 2], rtol=16 * 2.0 ** -24, atol=0)


def test_a_failed_step_leaves_the_epoch_state_untouched(gold):
    _, heat, heat_f, batch = gold
    step = PoseEvalStep(None, device="cuda")
    bad = dict(batch, keypoints=batch["keypoints"][:, :, :5])           # K of the keypoints != the heatmaps'
    with pytest.raises(AssertionError):
        step(bad, heatmaps=heat.cuda(), heatmaps_flipped=heat_f.cuda())
    assert step._seen == set() and step._slot_ids == [] and step.predictions() == []
    step(batch, heatmaps=heat.cuda(), heatmaps_flipped=heat_f.cuda())
    assert len(step.predictions()) == 7


def _loss_args(B=2, N=2, K=5, H=6, W=7):
    dev = "cuda"
    t = {"heat": torch.rand(B, K, H, W, device=dev), "flip": torch.rand(B, K, H, W, device=dev),
         "avg": torch.full((B, K, H, W), -7.0, device=dev), "kp": torch.rand(B, N, K, 3, device=dev),
         "per_kp": torch.full((B, K), -7.0, device=dev), "loss": torch.full((1,), -7.0, device=dev),
         "coords": torch.full((B, K, 2), -7.0, device=dev), "scores": torch.full((B, K), -7.0, device=dev)}
    return t, dict(B=B, N=N, K=K, H=H, W=W, topk=2)


def _call_loss(t, d, **over):
    a = dict(heat=t["heat"].data_ptr(), flip=t["flip"].data_ptr(), avg=t["avg"].data_ptr(), kp=t["kp"].data_ptr(),
             per_kp=t["per_kp"].data_ptr(), loss=t["loss"].data_ptr(), coords=t["coords"].data_ptr(),
             scores=t["scores"].data_ptr(), kpw=(C.c_float * 64)(*([1.0] * 64)), **d)
    a.update(over)
    return lib().prpe_pose_eval_loss(a["heat"], a["flip"], None, 0, a["avg"], a["B"], a["K"], a["H"], a["W"], a["kp"],
                                     None, None, a["N"], 2.0, a["kpw"], a["topk"], a["per_kp"], a["loss"],
                                     a["coords"], a["scores"], None, None, None, None)


@pytest.mark.parametrize("over", [dict(topk=6), dict(topk=0), dict(K=65, topk=2), dict(N=0), dict(heat=None),
                                  dict(kp=None), dict(kpw=None), dict(per_kp=None), dict(loss=None),
                                  dict(coords=None), dict(scores=None), "alias", "alias_offset", "heat_offset",
                                  dict(flip=None)],
                         ids=lambda o: o if isinstance(o, str) else ",".join(o))
def test_bad_arguments_return_einval_and_launch_nothing(over):
    t, d = _loss_args()
    if over == "alias":
        over = dict(avg=t["flip"].data_ptr())
    elif over == "alias_offset":
        over = dict(avg=t["flip"].data_ptr() + 64)                      # overlapping, not equal
    elif over == "heat_offset":
        over = dict(avg=t["heat"].data_ptr() + 64)                      # in place is fine, shifted is not
    flip_before = t["flip"].clone()
    assert _call_loss(t, d, **over) == -22                              # flip=None: avg_out without heat_flipped
    torch.cuda.synchronize()
    assert torch.equal(t["flip"], flip_before)
    for k in ("avg", "per_kp", "loss", "coords", "scores"):
        assert bool((t[k] == -7.0).all()), k
    assert _call_loss(t, d) == 0                                        # the same call, good arguments
    torch.cuda.synchronize()
    avg = t["avg"].clone()
    assert _call_loss(t, d, avg=t["heat"].data_ptr()) == 0              # in place
    assert torch.equal(t["heat"], avg)
    torch.cuda.synchronize()
    assert not bool((t["per_kp"] == -7.0).any()) and not bool((t["avg"] == -7.0).any())


def test_records_bad_arguments_return_einval():
    dev = "cuda"
    B, N, K = 2, 2, 5
    coords, scores = torch.rand(B, K, 2, device=dev), torch.rand(B, K, device=dev)
    boxes, areas = torch.rand(B, N, 4, device=dev), torch.rand(B, N, device=dev)
    masks = torch.ones(B, N, dtype=torch.uint8, device=dev)
    crowd = torch.zeros(B, N, dtype=torch.uint8, device=dev)
    keep = (C.c_uint8 * B)(*([1] * B))                               # a host array
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    kpts, meta = torch.full((8, K, 3), -7.0, device=dev), torch.full((8, 8), -7.0, device=dev)
    ptrs = [t.data_ptr() for t in (coords, scores, boxes, areas, masks, crowd)] + [C.cast(keep, C.c_void_p)]

    def call(ptrs=ptrs, B=B, N=N, K=K, counter_p=counter.data_ptr(), kp=kpts.data_ptr(), mp=meta.data_ptr()):
        return lib().prpe_pose_coco_records(*ptrs, B, N, K, 0.3, 0, counter_p, kp, mp, 8, None)
    assert call(K=65) == -22 and call(N=0) == -22 and call(B=0) == -22
    assert call(counter_p=None) == -22 and call(kp=None) == -22 and call(mp=None) == -22
    for i in range(len(ptrs)):
        assert call(ptrs=ptrs[:i] + [None] + ptrs[i + 1:]) == -22
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and bool((kpts == -7.0).all()) and bool((meta == -7.0).all())
    assert call() == 0
    assert int(counter.item()) == B * N


@pytest.fixture(scope="module")
def model(state_dict):
    return CombinedModel(state_dict, device="cuda")


def test_pose_eval_step_end_to_end_vs_unfused_chain(model):
    """PoseEvalStep on the model == pose_flip_test, then the restatement's target and loss in torch
    on the GPU, then prpe_softargmax and the record loop (GPU against GPU)."""
    B, N, K = 2, 3, 17
    x = synth.frames(B).cuda()
    avg = pose_flip_test(model, x, "reference")
    H, W = avg.shape[2:]
    _, _, kp, areas, boxes = T.random_case(13, B, N, K, H, W)
    kp[..., :2] = kp[..., :2].clamp(0.05, 0.95)
    kp[1, :, :, 2] = kp[0, :, :, 2].flip(0)                              # frame 1 visible too
    masks = torch.tensor([[True, True, False], [True, True, True]])
    crowd = torch.tensor([[False, False, False], [False, True, False]])
    batch = {"images": x, "keypoints": kp.cuda(), "boxes": boxes.cuda(), "areas": areas.cuda(), "masks": masks.cuda(),
             "is_crowd": crowd.cuda(), "image_ids": [7, 9]}
    step = PoseEvalStep(model, heatmap_size=(H, W))
    loss = step(batch)
    preds = step.predictions()
    # the unfused chain
    target, weights = T.ref_target(kp.cuda(), areas.cuda(), H, W, 2.0)
    l32 = float(T.ref_loss(avg, target, weights, KPW, 8)[0])
    t64, w64 = T.ref_target(kp.cuda(), areas.cuda(), H, W, 2.0, torch.float64)
    l64 = float(T.ref_loss(avg.double(), t64, w64, KPW, 8)[0])
    d = abs(float(loss) - l64)
    print(f"end to end: fused {float(loss):.9g} unfused fp32 {l32:.9g} fp64 {l64:.12g} distance {d:.3g}")
    assert d <= max(4 * abs(l32 - l64), 16 * ulp32(l64))
    c, s = ops.softargmax(avg, boxes[:, 0].cuda())
    assert torch.equal(step.last["coords"], c) and torch.equal(step.last["scores"], s)
    rk, rm = T.ref_records(c.cpu().numpy(), s.cpu().numpy(), boxes, areas, masks, crowd, [1, 1], 0.3)
    ref = format_coco_records(rk, rm, [7, 9])
    assert len(preds) == len(ref) == 4
    for p, r in zip(preds, ref):
        assert p["image_id"] == r["image_id"] and p["keypoints"] == r["keypoints"]
        assert p["bbox"] == r["bbox"] and p["area"] == r["area"]
        assert abs(p["score"] - r["score"]) <= 16 * ulp32(r["score"])
