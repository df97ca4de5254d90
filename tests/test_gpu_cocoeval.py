"""GPU: COCO keypoint AP / AR on the device (csrc/cocoeval.hip: prpe_coco_kp_match,
prpe_coco_kp_accumulate; PoseEvalStep.compute) against the host statement of COCOeval in
tests/test_coco_kp_host.py. Bounds: match / ignore bits, kept order and npig exact; OKS within
4 K 2^-53 (K terms <= 1, each off by at most the two 1-ulp exps, plus the summation order);
precision and recall bit-equal (correctly rounded quotients of the same integer counts); stats
within 1e-12 (a mean of <= 3030 values in [0, 1] in another order: <= 3030 * 2^-53 = 3.4e-13).
Every scenario passes ``check_input_condition`` on the CPU first, so a 1-ulp exp cannot flip a match.
"""
import numpy as np
import pytest
import torch

import test_coco_kp_host as H
import test_pose_eval_host as T
from prpe import CocoKeypointGT, PoseEvalStep, coco_keypoint_eval, ops
from prpe._lib import PrpeError
from prpe.evalsteps import (COCO_IOU_THRS, COCO_KP_AREA_RNGS, COCO_KP_STAT_KEYS, COCO_REC_THRS)

match_op = ops.coco_kp_match          # the module fails here without the kernels
pytestmark = pytest.mark.gpu


def _upload(gt, dets, K, pad=3):
    kp, meta, slot_ids = H.records_from_dets(dets, K)
    n = kp.shape[0]
    rec_kpts = torch.full((n + pad, K, 3), -7.0, device="cuda")
    rec_meta = torch.full((n + pad, 8), -7.0, device="cuda")
    rec_kpts[:n] = torch.from_numpy(kp).cuda()
    rec_meta[:n] = torch.from_numpy(meta).cuda()
    counter = torch.tensor([n], dtype=torch.int64, device="cuda")
    return rec_kpts, rec_meta, counter, n, slot_ids


def device_eval(name):
    gt, dets, K, _ = H.scenario(name)
    rec_kpts, rec_meta, counter, n, slot_ids = _upload(gt, dets, K)
    ev = coco_keypoint_eval(rec_kpts, rec_meta, counter, n + 3, slot_ids, gt, sigmas=H.sigmas_for(K))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in ev.items()}


def assert_equals_host(dev, gt, ref, K):
    want = H.tables(gt, ref)
    assert np.array_equal(dev["dt_rec"], want["dt_rec"])                        # kept detections, in order
    assert np.array_equal(dev["dt_bits"].view(np.uint64), want["dt_bits"])      # matched / ignored / empty
    assert np.array_equal(dev["npig"], want["npig"])
    assert np.array_equal(dev["dt_score"], want["dt_score"].astype(np.float32), equal_nan=True)
    hole = want["oks"] == -1.0
    assert np.array_equal(dev["oks"] == -1.0, hole)
    err = np.abs(dev["oks"] - want["oks"])[~hole]
    bound = 4 * K * 2.0 ** -53
    print(f"max |oks - host| = {err.max() if err.size else 0.0:.3e} (bound {bound:.3e})")
    assert not err.size or err.max() <= bound
    assert np.array_equal(dev["precision"].view(np.uint64), ref["precision"].view(np.uint64))
    assert np.array_equal(dev["recall"].view(np.uint64), ref["recall"].view(np.uint64))
    d = np.abs(dev["stats"] - ref["stats"]).max()
    print(f"max |stats - host| = {d:.3e}")
    assert d <= 1e-12


@pytest.mark.parametrize("name", H.scenario_names())
def test_device_equals_the_host_statement(name):
    gt, dets, K, ref = H.scenario(name)
    H.check_input_condition(ref)
    assert_equals_host(device_eval(name), gt, ref, K)


def test_two_runs_give_the_same_bits():
    a, b = device_eval("epoch64"), device_eval("epoch64")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_counter_bounds_the_records():
    """The device counter, not the host bound, says how many records there are; rows past it
    (here real records of another image) are not read."""
    gt, dets, K, _ = H.scenario("I")
    rec_kpts, rec_meta, counter, n, slot_ids = _upload(gt, dets, K, pad=0)
    counter.fill_(2)                                            # image 2's two records only
    ev = coco_keypoint_eval(rec_kpts, rec_meta, counter, n, slot_ids, gt)
    ref = H.coco_eval_loop(gt, dets[:2])
    assert_equals_host({k: v.cpu().numpy() for k, v in ev.items()}, gt, ref, K)
    ev = coco_keypoint_eval(rec_kpts, rec_meta, None, 2, slot_ids, gt)          # no counter: the host bound
    assert np.array_equal(ev["precision"].cpu().numpy(), ref["precision"])


def _sentinel_match_out(I):
    return {"dt_score": torch.full((I, 20), -7.0, device="cuda"),
            "dt_bits": torch.full((I, 20), -7, device="cuda", dtype=torch.int64),
            "dt_rec": torch.full((I, 20), -7, device="cuda", dtype=torch.int32),
            "npig": torch.full((I, 3), -7, device="cuda", dtype=torch.int32),
            "oks": torch.full((I, 20, 64), -7.0, device="cuda", dtype=torch.float64)}


def test_refusals_leave_outputs_untouched():
    gt, dets, K, _ = H.scenario("B")
    rec_kpts, rec_meta, counter, n, slot_ids = _upload(gt, dets, K)
    t = gt.to("cuda").tensors()
    s2i = torch.from_numpy(gt.slot_to_img(slot_ids)).cuda()
    out = _sentinel_match_out(len(gt))

    def call(max_gt=gt.max_gt, sig=H.sigmas_for(K), thr=COCO_IOU_THRS, n_max=n, kp=rec_kpts, gk=t["kpts"]):
        return ops.coco_kp_match(kp, rec_meta, counter, n_max, s2i, t["gt_start"], gk, t["bbox"], t["area"],
                                 t["iscrowd"], t["ignore"], max_gt, sig, thr, COCO_KP_AREA_RNGS, out=out)
    bad_sigma = H.sigmas_for(K).copy()
    bad_sigma[3] = 0.0
    nan_thr = COCO_IOU_THRS.copy()
    nan_thr[2] = np.nan
    for kw in (dict(max_gt=65), dict(sig=bad_sigma), dict(thr=nan_thr), dict(n_max=-1)):
        with pytest.raises(PrpeError, match="-22"):
            call(**kw)
    K65 = 65
    with pytest.raises(PrpeError, match="-22"):
        call(sig=H.sigmas_for(K65), kp=torch.zeros(n + 3, K65, 3, device="cuda"),
             gk=torch.zeros(t["kpts"].shape[0], K65, 3, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        call(n_max=n + 4)                                       # past the arrays: refused on the host
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == -7).all(), k
    call()
    acc = {"precision": torch.full((10, 101, 3), -7.0, device="cuda", dtype=torch.float64),
           "recall": torch.full((10, 3), -7.0, device="cuda", dtype=torch.float64),
           "stats": torch.full((10,), -7.0, device="cuda", dtype=torch.float64)}
    for bad in (COCO_REC_THRS[::-1], np.where(np.arange(101) == 4, np.nan, COCO_REC_THRS),
                np.where(np.arange(101) == 4, COCO_REC_THRS[3], COCO_REC_THRS)):
        with pytest.raises(PrpeError, match="-22"):
            ops.coco_kp_accumulate(out["dt_score"], out["dt_bits"], out["npig"], bad, out=acc)
    torch.cuda.synchronize()
    for k, v in acc.items():
        assert (v == -7).all(), k


# ------------------------------------------------------------------ PoseEvalStep.compute end to end
def _batch_annotations(batch, image_ids, seen):
    """The batch's own boxes and keypoints as COCO annotations in image pixels (the frames whose
    image id is new, as the record loop keeps them)."""
    anns = []
    kp, boxes, areas = batch["keypoints"].double(), batch["boxes"].double(), batch["areas"].double()
    for b, iid in enumerate(image_ids):
        if iid in seen:
            continue
        seen.add(iid)
        for n in range(kp.shape[1]):
            x1, y1, x2, y2 = boxes[b, n].tolist()
            k = kp[b, n].clone()
            k[:, 0] = k[:, 0] * (x2 - x1) + x1
            k[:, 1] = k[:, 1] * (y2 - y1) + y1
            anns.append(H.ann(iid, k.numpy(), bbox=[x1, y1, x2 - x1, y2 - y1], area=float(areas[b, n]),
                              iscrowd=int(batch["is_crowd"][b, n])))
    return anns


@pytest.fixture(scope="module")
def epoch():
    heat, heat_f, batch = T.pose_eval_inputs()
    ids2 = [104, 101, 105, 106]                                 # the second batch repeats image 101
    seen = set()
    anns = _batch_annotations(batch, batch["image_ids"], seen) + _batch_annotations(batch, ids2, seen)
    gt = CocoKeypointGT.from_annotations(anns)

    def run(capacity):
        step = PoseEvalStep(None, device="cuda", capacity=capacity)
        step(batch, heatmaps=heat.cuda(), heatmaps_flipped=heat_f.cuda())
        step(dict(batch, image_ids=ids2), heatmaps=heat.cuda(), heatmaps_flipped=heat_f.cuda())
        return step
    return gt, run


def test_pose_eval_step_compute_equals_the_host_statement_on_predictions(epoch):
    gt, run = epoch
    step = run(1 << 10)
    preds = step.predictions()
    assert len(preds) == 14 and int(step._state[0].item()) == 14             # two batches, frame 1 of the second dropped
    ref = H.coco_eval_loop(gt, preds)
    H.check_input_condition(ref)
    out = step.compute(gt)
    assert tuple(out) == COCO_KP_STAT_KEYS and all(isinstance(v, float) for v in out.values())
    dev = {k: v.cpu().numpy() for k, v in step.last_eval.items()}
    assert np.array_equal(np.array(list(out.values())), dev["stats"])
    assert_equals_host(dev, gt, ref, 17)
    assert step.predictions() == preds                          # compute leaves the records as they are


def test_records_at_capacity(epoch):
    gt, run = epoch
    full = run(1 << 10).compute(gt)
    assert run(14).compute(gt) == full                          # exactly full: no overflow
    with pytest.raises(RuntimeError, match="exceed the capacity"):
        run(13).compute(gt)


def test_compute_before_any_batch_counts_every_person_as_missed(epoch):
    gt, _ = epoch
    out = PoseEvalStep(None, device="cuda").compute(gt)
    assert out["val/AP"] == 0.0 and out["val/AR"] == 0.0


def test_compute_refuses_an_image_the_annotations_do_not_know(epoch):
    gt, run = epoch
    step = run(1 << 10)
    step(dict(T.pose_eval_inputs()[2], image_ids=[900, 901, 902, 903]), heatmaps=T.pose_eval_inputs()[0].cuda(),
         heatmaps_flipped=T.pose_eval_inputs()[1].cuda())
    with pytest.raises(ValueError, match="image id 900"):
        step.compute(gt)
