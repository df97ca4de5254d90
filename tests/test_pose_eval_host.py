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
import pytest
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


# ----------------------------------------------------------------------------- the edges
def _edge_base(seed, B, N, K, H, W, vis_lo=1.0):
    """Random heatmaps and keypoints with every keypoint drawn (visibility 1 or 2)."""
    heat = synth.uniform(seed, "edge_heat", (B, K, H, W), -1.0, 3.0)
    heat_f = synth.uniform(seed, "edge_heat_flipped", (B, K, H, W), -1.0, 3.0)
    xy = synth.uniform(seed, "edge_xy", (B, N, K, 2), 0.1, 0.9)
    vis = torch.floor(synth.uniform(seed, "edge_vis", (B, N, K)) * 2.0) + vis_lo
    areas = synth.uniform(seed, "edge_areas", (B, N), 3000.0, 30000.0)
    boxes = synth.uniform(seed, "edge_boxes", (B, N, 4)) * 100.0
    boxes[..., 2:] += boxes[..., :2] + 5.0
    return dict(heat=heat, heat_f=heat_f, kp=torch.cat([xy, vis[..., None]], -1), areas=areas, boxes=boxes,
                sigma=2.0, topk=min(2, K), pairs=[(1, 2)] if K > 2 else [], mode="reference",
                kpw=[1.0 + 0.25 * (k % 7) for k in range(K)])


F32 = torch.float32
CLAMP_AREAS = [2304.0, float(torch.nextafter(torch.tensor(2304.0), torch.tensor(1e9))), 36864.0,
               float(torch.nextafter(torch.tensor(36864.0), torch.tensor(0.0))), 0.0, -100.0, 9216.0]


def pose_edge_case(name):
    """The pose_eval_loss edge cases of tests/test_gpu_framestages.py (inputs only; this file pins
    the restatement on them). A dict: heat, heat_f [B,K,H,W], kp [B,N,K,3], areas [B,N] or None,
    boxes [B,N,4], sigma, topk, pairs, mode, kpw."""
    if name in ("reg_4096", "reg_4097"):
        # the register path's last size and the re-reading path's first, same streams: frame 0's
        # keypoint 0 is drawn by no instance (target 0, weight 0.5) and its maps hold the same
        # 4096 values (+ one 0), symmetric under the flip, so HW * per_kp[0, 0] is the same sum
        H, W = (64, 64) if name == "reg_4096" else (17, 241)
        c = _edge_base(41, 2, 3, 3, H, W)
        c["kp"][0, :, 0, 2] = 0.0
        v = synth.uniform(41, "edge_shared_map", (4096,), -1.0, 3.0)
        flat = torch.zeros(H * W)
        flat[:4096] = v
        c["heat"][0, 0] = flat.view(H, W)
        c["heat_f"][0, 0] = flat.view(H, W).flip(-1)
        return c
    if name == "map_256":
        return _edge_base(42, 2, 2, 3, 16, 16)
    if name == "map_35":
        return _edge_base(43, 3, 2, 4, 5, 7)
    if name == "map_1x1":
        c = _edge_base(44, 2, 2, 3, 1, 1)
        c["kp"][1, :, 1, 2] = 0.0                     # one map with no drawn keypoint
        return c
    if name in ("n_64", "n_65", "n_256"):
        N = int(name[2:])
        c = _edge_base(45, 2, N, 4, 8, 6, vis_lo=0.0)   # visibilities 0 and 1: no weight 1 ...
        c["kp"][0, N - 1, 2, 2] = 2.0                 # ... but from the last instance (n >= 192 at N = 256)
        c["kp"][1, 0, 1, 2] = 2.0
        c["kp"][1, 3] = c["kp"][1, 3] * torch.tensor([1.0, 1.0, 0.0])        # a skipped instance
        return c
    if name == "visibility":
        # values other than 0, 1, 2: 0.5 and 3 draw with weight 0.5, -1 does not draw; frame 1 has
        # no visible keypoint at all (weight 0); in frame 2 a skipped instance with NaN
        # coordinates and a negative area stands beside a visible one and changes nothing
        c = _edge_base(46, 3, 2, 4, 6, 5)
        c["kp"][0, :, :, 2] = torch.tensor([[0.5, 3.0, -1.0, 0.0], [0.0, 0.0, -1.0, 2.0]])
        c["kp"][1, :, :, 2] = torch.tensor([[0.0, -1.0, 0.0, -2.0], [0.0, 0.0, 0.0, 0.0]])
        c["kp"][2, 0] = torch.tensor([float("nan"), float("nan"), 0.0])
        c["areas"][2, 0] = -5.0
        c["kp"][2, 1, :, 2] = torch.tensor([1.0, 2.0, 1.0, 2.0])
        return c
    if name == "area_clamp":
        # sqrt(area) / 96 exactly 0.5 and 2, the next floats inside, area 0, a negative area (NaN
        # sigma: every map of that frame thresholds to zero, also where that instance's
        # visibility is 0 and the other instance draws) and one unclamped; boxes[:, 0] (the
        # score scale) span the same areas
        c = _edge_base(47, 7, 2, 3, 12, 9)
        side = torch.tensor(CLAMP_AREAS).abs().sqrt()
        c["areas"][:, 0] = torch.tensor(CLAMP_AREAS)
        c["boxes"][:, 0] = torch.stack([torch.full((7,), 3.0), torch.full((7,), 2.0), 3.0 + side, 2.0 + side], 1)
        c["boxes"][1, 0] = torch.tensor([0.0, 0.0, 1.0, CLAMP_AREAS[1]])
        c["boxes"][3, 0] = torch.tensor([0.0, 0.0, 1.0, CLAMP_AREAS[3]])
        c["boxes"][4, 0] = torch.tensor([7.0, 7.0, 7.0, 50.0])               # area 0
        c["boxes"][5, 0] = torch.tensor([9.0, 0.0, 4.0, 20.0])               # area -100
        c["kp"][5, 0, :, 2] = torch.tensor([0.0, 2.0, 1.0])
        c["kp"][5, 1, :, 2] = torch.tensor([2.0, 1.0, 1.0])
        return c
    if name == "centres":
        # a centre exactly on pixel (3, 2) (mu = 3.0, 2.0), one far outside the map (every
        # Gaussian underflows: sum 0, so the map is 0 / 1e-8 = 0), the rest random
        c = _edge_base(48, 2, 1, 3, 6, 8)
        c["areas"] = None
        c["kp"][0, 0, 0] = torch.tensor([3.5 / 8, 2.5 / 6, 2.0])
        c["kp"][0, 0, 1] = torch.tensor([50.0, -40.0, 2.0])
        return c
    if name == "tiny_sigma":
        # sigma = 1e-3: 2 sigma^2 = 2e-6, so a centre off the pixels by 0.2 gives exp(-2e4) = 0
        # everywhere (sum 0, denominator 1e-8), and a centre exactly on a pixel gives one 1
        c = _edge_base(49, 2, 1, 3, 6, 8)
        c["areas"], c["sigma"] = None, 1e-3
        c["kp"][..., 0] = (torch.floor(c["kp"][..., 0] * 8) + 0.7) / 8
        c["kp"][..., 1] = (torch.floor(c["kp"][..., 1] * 6) + 0.7) / 6
        c["kp"][0, 0, 0] = torch.tensor([3.5 / 8, 2.5 / 6, 2.0])
        return c
    if name == "k_1":
        c = _edge_base(50, 3, 2, 1, 6, 5)
        c["topk"] = 1
        return c
    if name == "k_64":
        c = _edge_base(51, 2, 2, 64, 6, 5)
        c["topk"] = 64                                # topk == K: every keypoint counts
        c["pairs"] = [(1, 2), (62, 63)]
        return c
    if name == "topk_1":
        return dict(_edge_base(52, 2, 2, 5, 6, 5), topk=1)
    if name in ("self_partner_reference", "self_partner_swap"):
        c = _edge_base(53, 3, 2, 4, 6, 5)
        c["pairs"], c["mode"] = [(1, 1), (2, 3)], name.split("_")[2]
        return c
    if name in ("ohkm_9_frames", "ohkm_nan"):
        # nine frames (a wave walks three); frame 4 has no visible keypoint: five equal losses of 0
        c = _edge_base(54, 9, 2, 5, 6, 5)
        c["kp"][4, :, :, 2] = 0.0
        c["topk"] = 3
        if name == "ohkm_nan":
            c["kpw"][3] = float("nan")
        return c
    raise KeyError(name)


POSE_EDGES = ["reg_4096", "reg_4097", "map_256", "map_35", "map_1x1", "n_64", "n_65", "n_256", "visibility",
              "area_clamp", "centres", "tiny_sigma", "k_1", "k_64", "topk_1", "self_partner_reference",
              "self_partner_swap", "ohkm_9_frames", "ohkm_nan"]


def target_plain(kp, areas, H, W, sigma):
    """_generate_target_heatmap's rule pixel by pixel in Python floats (float64, math.exp), written
    apart from ``ref_target``: returns (maps before the threshold, thresholded maps, weights)."""
    import math
    kp = kp.double()
    B, N, K, _ = kp.shape
    nan = float("nan")
    pre = torch.zeros(B, K, H, W, dtype=torch.float64)
    weights = torch.zeros(B, K, dtype=torch.float64)

    def fmax(a, b):                                   # torch.maximum: a NaN on either side wins
        return nan if (a != a or b != b) else max(a, b)

    for b in range(B):
        heat = [[[0.0] * W for _ in range(H)] for _ in range(K)]
        wts = [0.0] * K
        for n in range(N):
            vis = [float(kp[b, n, k, 2]) for k in range(K)]
            if not any(v > 0 for v in vis):
                continue                              # the instance is skipped whole: no weight either
            sg = float(sigma)
            if areas is not None:
                a = float(areas[b, n])
                s = math.sqrt(a) / 96.0 if a >= 0 else nan
                sg = sigma * (s if s != s else min(max(s, 0.5), 2.0))
            for k in range(K):
                mx, my = float(kp[b, n, k, 0]) * W - 0.5, float(kp[b, n, k, 1]) * H - 0.5
                wts[k] = max(wts[k], 1.0 if vis[k] == 2 else 0.5)
                for y in range(H):
                    for x in range(W):
                        q = -((x - mx) ** 2 + (y - my) ** 2) / (2 * sg * sg)
                        g = nan if q != q else (math.exp(q) if q > -745.0 else 0.0)
                        g = g * (1.0 if vis[k] > 0 else 0.0)         # NaN * 0 = NaN, as in the reference
                        heat[k][y][x] = fmax(heat[k][y][x], g)
        h = torch.tensor(heat, dtype=torch.float64)
        pre[b] = h / (h.sum(dim=(1, 2), keepdim=True) + 1e-8)
        weights[b] = torch.tensor(wts, dtype=torch.float64)
    return pre, torch.where(pre > 0.005, pre, torch.zeros_like(pre)), weights


@pytest.mark.parametrize("name", ["map_35", "map_1x1", "visibility", "area_clamp", "centres", "tiny_sigma", "k_1",
                                  "topk_1"])
def test_ref_target_at_the_edges_equals_the_plain_statement(name):
    """``ref_target`` in float64 against ``target_plain`` on the small edge cases. Weights and the
    zero pattern agree exactly; values agree to 8 fp64 ulps of the map's peak (math.exp against
    torch.exp and another order of the sum). What the reference (module.py:336-378) does at the
    edges, read from its code: a visibility that is neither 2 nor <= 0 draws with weight 0.5; an
    instance with no visibility > 0 is skipped whole; sqrt of a negative area is NaN, clamp keeps
    a NaN, and the Gaussian times the visibility mask is NaN also where the mask is 0, so every
    map of that frame is NaN before the threshold and 0 after it; a sum of 0 divides by 1e-8."""
    c = pose_edge_case(name)
    H, W = c["heat"].shape[2:]
    pre, thr, wts = target_plain(c["kp"], c["areas"], H, W, c["sigma"])
    r_pre, r_w = ref_target(c["kp"], c["areas"], H, W, c["sigma"], torch.float64, thresholded=False)
    r_thr, _ = ref_target(c["kp"], c["areas"], H, W, c["sigma"], torch.float64)
    assert torch.equal(r_w, wts)
    assert torch.equal(torch.isnan(r_pre), torch.isnan(pre))
    assert torch.equal(r_thr != 0, thr != 0) and not bool(torch.isnan(r_thr).any())
    tol = 8 * 2.0 ** -52 * thr.amax(dim=(2, 3), keepdim=True)
    assert bool(((r_thr - thr).abs() <= tol).all())
    # the fp32 restatement draws the same maps (the GPU tests' yardstick)
    t32, w32 = ref_target(c["kp"], c["areas"], H, W, c["sigma"])
    assert torch.equal(w32.double(), wts) and not bool(torch.isnan(t32).any())
    if name == "visibility":
        assert wts.tolist() == [[0.5, 0.5, 0.5, 1.0], [0.0] * 4, [0.5, 1.0, 0.5, 1.0]]
        assert not bool(thr[1].any()) and bool(thr[0, 0].any()) and bool(thr[0, 1].any()) and not bool(thr[0, 2].any())
        assert not bool(torch.isnan(pre).any())       # the skipped instance's NaN and negative area are never read
    if name == "area_clamp":
        assert bool(torch.isnan(pre[5]).all()) and not bool(thr[5].any()) and wts[5].tolist() == [1.0, 1.0, 0.5]
        assert all(bool(thr[b].any()) for b in (0, 1, 2, 3, 4, 6))
        sg = 2.0 * torch.clamp(torch.sqrt(c["areas"][:, 0]) / 96.0, min=0.5, max=2.0)
        assert sg[0] == 1.0 and sg[2] == 4.0 and sg[4] == 1.0 and 1.0 < sg[1] < 1.0001 and 3.9999 < sg[3] < 4.0
    if name == "centres":
        assert float(thr[0, 0, 2, 3]) == float(thr[0, 0].max()) and not bool(thr[0, 1].any())
    if name == "tiny_sigma":
        one = torch.zeros(6, 8, dtype=torch.float64)
        one[2, 3] = 1.0 / (1.0 + 1e-8)
        assert torch.equal(thr[0, 0], one) and not bool(thr[0, 1:].any()) and not bool(thr[1].any())


@pytest.mark.parametrize("name", POSE_EDGES)
def test_edge_cases_meet_the_band_cap(name):
    """No pixel of an edge case lies within the target tolerance of the 0.005 threshold (the cap
    is 0.1 %; the streams were chosen for none), and the fp32 restatement's loss is finite unless
    the case is the NaN one: then torch.topk ranks the NaN first and the loss is NaN."""
    c = pose_edge_case(name)
    H, W = c["heat"].shape[2:]
    pre, _ = ref_target(c["kp"], c["areas"], H, W, c["sigma"], thresholded=False)
    n = int(band_mask(torch.nan_to_num(pre, nan=1.0)).sum())
    print(f"{name}: {n} of {pre.numel()} pixels in the band")
    assert n == 0
    avg = ref_flip_average(c["heat"], c["heat_f"], c["mode"], c["pairs"])
    target, weights = ref_target(c["kp"], c["areas"], H, W, c["sigma"])
    loss, per_kp = ref_loss(avg, target, weights, c["kpw"], c["topk"])
    assert bool(torch.isnan(loss)) == (name == "ohkm_nan")
    if name == "ohkm_nan":
        assert bool(torch.isnan(per_kp[:, 3]).all()) and not bool(torch.isnan(per_kp[:, [0, 1, 2, 4]]).any())
    if name == "ohkm_9_frames":
        assert not bool(per_kp[4].any()) and bool(per_kp[3].all())


def test_self_partner_flip_average():
    """partner[k] == k: the reference mode reverses the frames of every paired channel and moves no
    channel (flip(0) of the two copies it indexes, module.py:479-484), so a self-paired channel is
    treated like any paired one; the swap mode leaves a self-paired channel where it is."""
    c = pose_edge_case("self_partner_reference")
    f = torch.flip(c["heat_f"], dims=[-1])
    ref = ref_flip_average(c["heat"], c["heat_f"], "reference", c["pairs"])
    assert torch.equal(ref[:, 1], (c["heat"][:, 1] + f[:, 1].flip(0)) * 0.5)
    assert torch.equal(ref[:, 2], (c["heat"][:, 2] + f[:, 2].flip(0)) * 0.5)
    assert torch.equal(ref[:, 0], (c["heat"][:, 0] + f[:, 0]) * 0.5)
    swp = ref_flip_average(c["heat"], c["heat_f"], "swap", c["pairs"])
    assert torch.equal(swp[:, 1], (c["heat"][:, 1] + f[:, 1]) * 0.5)
    assert torch.equal(swp[:, 2], (c["heat"][:, 2] + f[:, 3]) * 0.5)


def ohkm_plain(per_kp, topk):
    """OHKM in Python floats: per frame the ``topk`` largest, a NaN above every number, ties by
    the lower index (the sum does not depend on which of two equal values is taken)."""
    total = 0.0
    for row in per_kp.tolist():
        order = sorted(range(len(row)), key=lambda k: (0 if row[k] != row[k] else 1, -row[k] if row[k] == row[k] else 0, k))
        total += sum(row[k] for k in order[:topk])
    return total / (len(per_kp) * topk)


def test_ref_loss_ohkm_with_ties_and_nan():
    """``ref_loss``'s selection against ``ohkm_plain`` in float64: all-equal losses, a NaN (first in
    torch.topk's order, so the loss is NaN whenever a frame holds one)."""
    per = torch.tensor([[0.0, 0.0, 0.0, 0.0], [3.0, 1.0, 3.0, 2.0], [0.5, 4.0, 0.25, 1.0]], dtype=torch.float64)
    for topk in (1, 2, 4):
        out = torch.ones(3, 4, 1, dtype=torch.float64)
        loss, got = ref_loss(out * per.sqrt()[..., None], torch.zeros_like(out), torch.ones(3, 4, dtype=torch.float64),
                             [1.0] * 4, topk)
        assert torch.equal(got, per.sqrt() ** 2)
        assert abs(float(loss) - ohkm_plain(got, topk)) <= 1e-15
    per[1, 3] = float("nan")
    for topk in (1, 3):
        top = torch.topk(per, topk, dim=1)[0]
        assert bool(torch.isnan(top[1, 0])) and not bool(torch.isnan(top[[0, 2]]).any())
        assert ohkm_plain(per, topk) != ohkm_plain(per, topk)


# name -> the pose_coco_records edge cases of tests/test_gpu_framestages.py
def records_edge_case(name):
    K = {"k_1": 1, "k_7": 7, "k_64": 64}.get(name, 5)
    B, N = 4, 4
    g = torch.Generator().manual_seed(61 + K)
    coords, scores = torch.rand(B, K, 2, generator=g), torch.rand(B, K, generator=g)
    boxes = torch.rand(B, N, 4, generator=g) * 50
    boxes[..., 2:] += boxes[..., :2] + 1
    areas = torch.rand(B, N, generator=g) * 1000
    masks = torch.ones(B, N, dtype=torch.bool)
    crowd = torch.zeros(B, N, dtype=torch.bool)
    masks[0] = torch.tensor([False, True, True, False])          # not a prefix: instances 0 and 1 all the same
    masks[2] = torch.tensor([True, False, True, True])           # instances 0, 1, 2
    crowd[1, 1] = True                                           # a crowd instance between two kept ones
    crowd[2, 0] = True
    keep = [1, 1, 1, 0] if name != "all_kept" else [1, 1, 1, 1]
    thr32 = torch.tensor(0.3, dtype=torch.float32)
    scores[0, 0] = thr32                                         # float32(0.3) > 0.3: v = 2
    if K > 1:
        scores[0, 1] = torch.nextafter(thr32, torch.tensor(0.0))  # v = 1
    return dict(coords=coords, scores=scores, boxes=boxes, areas=areas, masks=masks, crowd=crowd, keep=keep,
                thresh=0.3, want_order=[(0, 0), (0, 1), (1, 0), (1, 2), (1, 3), (2, 1), (2, 2)])


def records_plain(c, slot_base=0):
    """The record loop (module.py:505-561) one Python scalar at a time: [(image, instance, [x, y,
    v] * K, score, bbox, area)] with x, y as numpy float32 (a product, then a sum)."""
    f = np.float32
    out = []
    K = c["coords"].shape[1]
    for b in range(len(c["keep"])):
        if not c["keep"][b]:
            continue
        for n in range(int(c["masks"][b].sum())):
            if bool(c["crowd"][b, n]):
                continue
            x1, y1, x2, y2 = (f(v) for v in c["boxes"][b, n].tolist())
            kps = []
            for k in range(K):
                kx, ky, s = f(c["coords"][b, k, 0].item()), f(c["coords"][b, k, 1].item()), c["scores"][b, k].item()
                kps += [f(f(kx * f(x2 - x1)) + x1), f(f(ky * f(y2 - y1)) + y1), 2 if s > c["thresh"] else 1]
            mean = float(c["scores"][b].double().mean())
            out.append((slot_base + b, n, kps, mean, [x1, y1, x2, y2], f(c["areas"][b, n].item())))
    return out


@pytest.mark.parametrize("name", ["k_1", "k_5", "k_7", "k_64"])
def test_ref_records_at_the_edges_equals_the_plain_statement(name):
    """``ref_records`` against ``records_plain``: masks that are no prefix (range(masks.sum()): the
    first ``sum`` instances, module.py:516), a crowd instance between kept ones, a score exactly
    float32(0.3) against the double 0.3 (score.item() > 0.3 holds: v = 2; the float below gives
    1). Everything exact but the instance score (an fp32 mean against the float64 mean: 16 ulps;
    exact for K = 1)."""
    c = records_edge_case(name)
    kp, meta = ref_records(c["coords"].numpy(), c["scores"].numpy(), c["boxes"], c["areas"], c["masks"], c["crowd"],
                           c["keep"], c["thresh"], slot_base=9)
    plain = records_plain(c, slot_base=9)
    K = c["coords"].shape[1]
    assert [(p[0] - 9, p[1]) for p in plain] == c["want_order"] and len(kp) == len(meta) == len(plain)
    for r, (img, inst, kps, mean, bbox, area) in enumerate(plain):
        assert meta[r, :2].copy().view(np.int32).tolist() == [img, inst]
        assert np.array_equal(kp[r].reshape(-1), np.array(kps, np.float32))
        assert np.array_equal(meta[r, 3:7], np.array(bbox, np.float32)) and meta[r, 7] == area
        if K == 1:
            assert meta[r, 2] == np.float32(mean)
        assert abs(float(meta[r, 2]) - mean) <= 16 * float(np.spacing(np.float32(mean)))
    assert kp[0, 0, 2] == 2.0 and (K == 1 or kp[0, 1, 2] == 1.0)
