"""CPU: the pose validation step's host side, and the plain-torch restatement of the reference
functions that the GPU tests (tests/test_gpu_pose_eval.py) compare the kernels against.

tests/golden/golden_pose_eval.npz was made by tools/make_golden_pose_eval.py, which ran the
reference's ``PoseEstimationModule.validation_step`` (pose_estimation/module.py:451-570) as
written on ``pose_eval_inputs()`` with a stub model, capturing ``_generate_target_heatmap``'s and
``_get_keypoints_from_heatmaps``'s outputs, the returned val_loss and eval_predictions.

The restatement (``ref_target``, ``ref_loss``, ``ref_keypoints``) is dtype- and device-generic:
in fp32 on the CPU it must give the golden's target and weights bit for bit and its loss (this
file pins that); in fp64 it gives the fixture's ``val_loss_fp64``, the centre of the GPU loss
tolerance.
"""
import os

import numpy as np
import torch

from prpe import synth
from prpe.evalsteps import COCO_SIGMAS, PoseEvalStep, format_coco_records, joints_mse_keypoint_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_pose_eval.npz")
PRED_KEYS = ["image_id", "category_id", "keypoints", "score", "bbox", "area"]
BAND_ULPS = 4            # target tolerance, in fp32 ulps of a map's peak value
BAND_CAP = 1e-3          # at most 0.1 % of the pixels may sit that close to the 0.005 threshold


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ----------------------------------------------------------------------------- the inputs
def pose_eval_inputs():
    """The validation batch of golden_pose_eval.npz: B=4, N=3, K=17, 64x48 (bit-identical from
    prpe.synth's streams). Returns (heat, heat_flipped, batch)."""
    B, N, K, H, W = 4, 3, 17, 64, 48
    heat = synth.uniform(51, "pose_eval_heat", (B, K, H, W), -1.0, 3.0)
    heat_f = synth.uniform(51, "pose_eval_heat_flipped", (B, K, H, W), -1.0, 3.0)
    # a peak in some channels (at the mirrored column of the flipped pass): their scores pass the
    # keypoint threshold, the flat channels' do not, so the records hold v = 2 and v = 1
    heat[:, [0, 1, 2, 3, 10, 11], 20, 30] = 14.0
    heat_f[:, [0, 1, 2, 3, 10, 11], 20, W - 1 - 30] = 14.0
    xy = synth.uniform(51, "pose_eval_kp_xy", (B, N, K, 2), 0.05, 0.95)
    vis = torch.floor(synth.uniform(51, "pose_eval_kp_vis", (B, N, K)) * 3.0)      # 0, 1, 2
    areas = synth.uniform(51, "pose_eval_areas", (B, N), 500.0, 60000.0)
    boxes = synth.uniform(51, "pose_eval_boxes", (B, N, 4)) * 150.0
    boxes[..., 2:] = boxes[..., :2] + 20.0 + synth.uniform(51, "pose_eval_boxes_wh", (B, N, 2)) * 200.0
    masks = torch.ones(B, N, dtype=torch.bool)
    crowd = torch.zeros(B, N, dtype=torch.bool)
    # frame 0: visibilities 0, 1 and 2 within instance 0; an all-invisible padding instance
    # BETWEEN two valid ones, and a masks row with fewer true entries than N (the record loop
    # then visits instances 0 and 1: the count, not the positions); areas at both clamps and inside
    vis[0, 0, :3] = torch.tensor([0.0, 1.0, 2.0])
    vis[0, 1] = 0.0
    masks[0] = torch.tensor([True, False, True])
    areas[0] = torch.tensor([0.0, 2500.0, 160000.0])
    # frame 1: keypoints within half a pixel of each border and one outside the map; a keypoint
    # column with no visible instance (target 0, weight 0.5); areas on the clamp's edges
    xy[1, 0, :5] = torch.tensor([[0.004, 0.5], [0.996, 0.5], [0.5, 0.003], [0.5, 0.997], [1.08, -0.05]])
    vis[1, 0, :5] = 2.0
    vis[1, :, 5] = 0.0
    areas[1] = torch.tensor([2400.7, 9216.0, 36864.0])
    # frame 2: a crowd instance; frame 3 repeats frame 1's image id
    crowd[2, 1] = True
    image_ids = [101, 102, 103, 102]
    batch = {"images": synth.uniform(51, "pose_eval_images", (B, 3, 256, 192)),
             "keypoints": torch.cat([xy, vis[..., None]], -1), "boxes": boxes, "areas": areas, "masks": masks,
             "is_crowd": crowd, "image_ids": image_ids}
    return heat, heat_f, batch


def inputs_checksum(heat, heat_f, batch) -> float:
    s = heat.double().sum() + 3 * heat_f.double().sum()
    for i, k in enumerate(("keypoints", "boxes", "areas", "masks", "is_crowd")):
        s = s + (5 + 2 * i) * batch[k].double().sum()
    return float(s + sum(batch["image_ids"]))


def random_case(seed, B, N, K, H, W):
    """A small batch for the odd-shape tests: random keypoints / visibilities / areas, one
    all-invisible instance and (B > 1) one frame with no visible keypoint at all (weight 0)."""
    heat = synth.uniform(seed, "odd_heat", (B, K, H, W), -1.0, 3.0)
    heat_f = synth.uniform(seed, "odd_heat_flipped", (B, K, H, W), -1.0, 3.0)
    xy = synth.uniform(seed, "odd_xy", (B, N, K, 2), -0.1, 1.1)
    vis = torch.floor(synth.uniform(seed, "odd_vis", (B, N, K)) * 3.0)
    if N > 1:
        vis[0, N - 1] = 0.0
    if B > 1:
        vis[1] = 0.0
    areas = synth.uniform(seed, "odd_areas", (B, N), 0.0, 50000.0)
    boxes = synth.uniform(seed, "odd_boxes", (B, N, 4)) * 100.0
    boxes[..., 2:] += boxes[..., :2] + 5.0
    return heat, heat_f, torch.cat([xy, vis[..., None]], -1), areas, boxes


# ----------------------------------------------------------------------------- the restatement
def ref_flip_average(heat, heat_f, mode, pairs):
    """module.py:479-484 ("reference"), or the channel swap the code intends ("swap")."""
    f = torch.flip(heat_f, dims=[-1]).clone()
    for a, b in pairs:
        if mode == "reference":
            f[:, [a, b]] = f[:, [a, b]].flip(0)
        else:
            f[:, [a, b]] = f[:, [b, a]]
    return (heat + f) * 0.5


def ref_target(keypoints, areas, H, W, sigma, dtype=torch.float32, thresholded=True):
    """_generate_target_heatmap (module.py:298-380), the instance loop kept, the frames batched
    (every operation is elementwise per frame, so the values are the loop's). keypoints
    [B,N,K,3]; returns (heatmaps [B,K,H,W], weights [B,K])."""
    kp = keypoints.to(dtype)
    dev = kp.device
    B, N, K, _ = kp.shape
    vis = kp[..., 2]
    heat = torch.zeros(B, K, H, W, dtype=dtype, device=dev)
    weights = torch.zeros(B, K, dtype=dtype, device=dev)
    y_grid, x_grid = torch.meshgrid(torch.arange(H, dtype=dtype, device=dev),
                                    torch.arange(W, dtype=dtype, device=dev), indexing="ij")
    mu_x = kp[..., 0] * W - 0.5
    mu_y = kp[..., 1] * H - 0.5
    if areas is not None:
        sg = sigma * torch.clamp(torch.sqrt(areas.to(dtype)) / 96.0, min=0.5, max=2.0)
    else:
        sg = torch.full((B, N), sigma, dtype=dtype, device=dev)
    for n in range(N):
        valid = vis[:, n] > 0                                        # [B,K]
        proc = valid.any(dim=1)                                      # `continue` where none (:348-350)
        dx = x_grid[None, None] - mu_x[:, n, :, None, None]
        dy = y_grid[None, None] - mu_y[:, n, :, None, None]
        g = torch.exp(-(dx.pow(2) + dy.pow(2)) / (2 * sg[:, n, None, None, None].pow(2))) * valid[:, :, None, None]
        heat = torch.where(proc[:, None, None, None], torch.maximum(heat, g), heat)
        w = torch.where(vis[:, n] == 2, torch.ones_like(weights), 0.5 * torch.ones_like(weights))
        weights = torch.where(proc[:, None], torch.maximum(weights, w), weights)
    heat = heat / (heat.sum(dim=(2, 3), keepdim=True) + 1e-8)
    if not thresholded:
        return heat, weights
    return torch.where(heat > 0.005, heat, torch.zeros_like(heat)), weights


def ref_loss(output, target, target_weight, kp_weights, topk):
    """JointsMSELoss.forward with target weights and OHKM (module.py:60-111). Returns (loss,
    per-keypoint loss [B,K] before the OHKM mask)."""
    B, K = output.shape[:2]
    kw = torch.as_tensor(kp_weights).to(device=output.device, dtype=output.dtype)
    combined = target_weight * kw.view(1, -1)
    loss = ((output.reshape(B, K, -1) - target.reshape(B, K, -1)) ** 2).mean(dim=2) * combined
    idx = torch.topk(loss, k=topk, dim=1)[1]
    mask = torch.zeros_like(loss)
    for i in range(B):
        mask[i, idx[i]] = 1
    return (loss * mask).sum() / (B * topk), loss


def ref_keypoints(heatmaps, boxes=None):
    """_get_keypoints_from_heatmaps (module.py:237-296); boxes [B,4]."""
    B, K, H, W = heatmaps.shape
    dev, dt = heatmaps.device, heatmaps.dtype
    y_grid, x_grid = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev),
                                    indexing="ij")
    prob = torch.softmax(heatmaps.reshape(B, K, -1), dim=2).reshape(B, K, H, W)
    x = (prob * x_grid[None, None]).sum(dim=(2, 3)) + 0.5
    y = (prob * y_grid[None, None]).sum(dim=(2, 3)) + 0.5
    scores = prob.reshape(B, K, -1).max(dim=2)[0]
    coords = torch.stack([x / W, y / H], dim=-1)
    if boxes is not None:
        a = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        scores = scores * torch.clamp(torch.sqrt(a).view(-1, 1) / 96.0, min=0.5, max=2.0)
    return coords, scores


def ref_val_loss(heat, heat_f, batch, dtype, mode="reference", sigma=2.0, topk=8):
    """The step's val_loss from the two heatmaps, every function in ``dtype``."""
    from prpe.evalsteps import COCO_FLIP_PAIRS
    avg = ref_flip_average(heat.to(dtype), heat_f.to(dtype), mode, COCO_FLIP_PAIRS)
    H, W = heat.shape[2:]
    target, weights = ref_target(batch["keypoints"], batch["areas"], H, W, sigma, dtype)
    return ref_loss(avg, target, weights, joints_mse_keypoint_weights(), topk)[0]


def ref_records(coords, scores, boxes, areas, masks, crowd, keep, thresh, slot_base=0):
    """The record loop (module.py:505-561) as fp32 numpy arrays (rec_kpts [n,K,3], rec_meta [n,8])
    in the device layout: x = kx * (x2 - x1) + x1 with two fp32 roundings."""
    c, s, bx, ar = (np.asarray(t, dtype=np.float32) for t in (coords, scores, boxes, areas))
    kp, meta = [], []
    for b in range(c.shape[0]):
        if not keep[b]:
            continue
        for n in range(int(np.asarray(masks[b]).sum())):
            if crowd[b][n]:
                continue
            x1, y1, x2, y2 = bx[b, n]
            x = c[b, :, 0] * (x2 - x1) + x1
            y = c[b, :, 1] * (y2 - y1) + y1
            v = np.where(s[b].astype(np.float64) > thresh, 2.0, 1.0).astype(np.float32)
            kp.append(np.stack([x, y, v], -1))
            ints = np.array([slot_base + b, n], dtype=np.int32).view(np.float32)
            meta.append(np.concatenate([ints, np.array([s[b].mean(dtype=np.float32), x1, y1, x2, y2, ar[b, n]],
                                                       dtype=np.float32)]))
    K = c.shape[1]
    return (np.stack(kp) if kp else np.zeros((0, K, 3), np.float32),
            np.stack(meta) if meta else np.zeros((0, 8), np.float32))


def band_mask(pre_threshold, ulps=BAND_ULPS):
    """Pixels whose value before thresholding lies within ``ulps`` fp32 ulps of the map's peak
    of 0.005: there a value that differs by that much may fall on the other side."""
    pre = torch.as_tensor(pre_threshold)
    tol = target_tolerance(pre, ulps)
    return (pre - 0.005).abs() <= tol


def target_tolerance(target, ulps=BAND_ULPS):
    """``ulps`` fp32 ulps of each (b, k) map's peak value, [B,K,1,1]."""
    peak = torch.as_tensor(target).amax(dim=(2, 3), keepdim=True)
    exp = torch.floor(torch.log2(peak.clamp(min=2.0 ** -126)))
    return ulps * torch.pow(2.0, exp - 23)


def golden_predictions(g):
    """The golden's eval_predictions as the reference's list of dicts."""
    out = []
    for r in range(len(g["pred_image_id"])):
        kp = g["pred_keypoints"][r].tolist()
        kp[2::3] = [int(v) for v in kp[2::3]]
        out.append(dict(zip([str(k) for k in g["pred_keys"]],
                            [int(g["pred_image_id"][r]), int(g["pred_category_id"][r]), kp, float(g["pred_score"][r]),
                             g["pred_bbox"][r].tolist(), float(g["pred_area"][r])])))
    return out


# ----------------------------------------------------------------------------- the tests
def test_inputs_are_the_goldens():
    g = load_golden()
    heat, heat_f, batch = pose_eval_inputs()
    assert inputs_checksum(heat, heat_f, batch) == float(g["input_sum"])
    kp = batch["keypoints"]
    assert set(kp[0, 0, :, 2].tolist()) == {0.0, 1.0, 2.0}
    assert not kp[0, 1, :, 2].any() and kp[0, 0, :, 2].any() and kp[0, 2, :, 2].any()
    assert not kp[1, :, 5, 2].any()
    assert int(batch["masks"][0].sum()) < kp.shape[1] and bool(batch["is_crowd"].any())
    assert len(set(batch["image_ids"])) < len(batch["image_ids"])


def test_restatement_reproduces_the_reference_target_weights_and_loss():
    g = load_golden()
    heat, heat_f, batch = pose_eval_inputs()
    H, W = heat.shape[2:]
    target, weights = ref_target(batch["keypoints"], batch["areas"], H, W, 2.0)
    assert np.array_equal(target.numpy(), g["target"])
    assert np.array_equal(weights.numpy(), g["weights"])
    assert float((g["target"][1, 5] != 0).sum()) == 0 and g["weights"][1, 5] == 0.5     # no visible instance
    assert ref_val_loss(heat, heat_f, batch, torch.float32).item() == float(g["val_loss"])
    assert ref_val_loss(heat, heat_f, batch, torch.float64).item() == float(g["val_loss_fp64"])
    from prpe.evalsteps import COCO_FLIP_PAIRS
    avg = ref_flip_average(heat, heat_f, "reference", COCO_FLIP_PAIRS)
    c, s = ref_keypoints(avg, batch["boxes"][:, 0])
    assert np.array_equal(c.numpy(), g["coords"]) and np.array_equal(s.numpy(), g["scores"])


def test_fixture_meets_the_band_cap():
    """At most 0.1 % of the golden's pixels lie within the target tolerance of the 0.005
    threshold (the GPU test lets only those differ by being zero on one side)."""
    heat, _, batch = pose_eval_inputs()
    pre, _ = ref_target(batch["keypoints"], batch["areas"], *heat.shape[2:], 2.0, thresholded=False)
    n = int(band_mask(pre).sum())
    assert n <= BAND_CAP * pre.numel(), n


def test_keypoint_weights_equal_the_references():
    g = load_golden()
    w = joints_mse_keypoint_weights()
    assert w.dtype == np.float32 and np.array_equal(w, g["kp_weights"])
    assert np.array_equal(PoseEvalStep(device="cpu").kp_weights, g["kp_weights"])
    assert COCO_SIGMAS.dtype == np.float32 and np.array_equal(COCO_SIGMAS, g["coco_sigmas"])


def test_prediction_records_format_like_the_reference():
    """predictions()'s formatting on record arrays built from the golden's own coords / scores:
    the reference's dicts, key order and types included, the repeated image id dropped."""
    g = load_golden()
    _, _, batch = pose_eval_inputs()
    step = PoseEvalStep(device="cpu")
    keep = step.keep_flags(batch["image_ids"])
    assert keep == [1, 1, 1, 0]
    assert step.keep_flags([103, 104]) == [0, 1]                       # a later batch of the epoch
    kp, meta = ref_records(g["coords"], g["scores"], batch["boxes"], batch["areas"], batch["masks"],
                           batch["is_crowd"], keep, 0.3)
    preds = format_coco_records(kp, meta, step._slot_ids)
    ref = golden_predictions(g)
    assert len(preds) == len(ref) == 7
    assert 102 in [p["image_id"] for p in preds] and [p["image_id"] for p in preds].count(102) == 3
    for p, r in zip(preds, ref):
        assert list(p.keys()) == PRED_KEYS == list(r.keys())
        assert p["image_id"] == r["image_id"] and p["category_id"] == 1 and type(p["image_id"]) is int
        assert p["keypoints"] == r["keypoints"]
        assert all(type(v) is int for v in p["keypoints"][2::3]) and set(p["keypoints"][2::3]) == {1, 2}
        assert all(type(v) is float for v in p["keypoints"][0::3] + p["keypoints"][1::3])
        assert p["bbox"] == r["bbox"] and p["area"] == r["area"]
        assert abs(p["score"] - r["score"]) <= 16 * 2.0 ** -24 * abs(r["score"])
    step.reset()
    assert step.keep_flags([102]) == [1]
