"""GPU: tracking persons across frames (csrc/track.hip, prpe.tracks) -- prpe_track_update against
``track_update_ref`` of tests/test_tracks_host.py (which a second, separately written statement
agrees with on every scenario), and ``PersonTracker`` against its stages run apart.

Tolerance: none. The tracker's arithmetic is fp32 sums, products and quotients that round once
each, on both sides, and everything else is integers: every output array and every state array is
compared bit for bit, after every call of every scenario (a scenario's calls run one after the
other on the device's own state). The scenarios are small on purpose: at most 40 frames, 70 person
slots and 3 streams; the capacity case fills the 32 x 32 key matrix."""
import pytest
import torch

import test_tracks_host as TH
from prpe import CombinedModel, FaceGallery, PersonRecognition, PersonTracker, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
MODES = {0: "iou", 1: "pose"}


def _sentinels(P, B):
    return (torch.full((P,), 77, device=DEV, dtype=torch.int32), torch.full((P,), 77, device=DEV, dtype=torch.int32),
            torch.full((P,), 77, device=DEV, dtype=torch.int64), torch.full((P,), 7.0, device=DEV),
            torch.full((B,), 77, device=DEV, dtype=torch.int32))


def device_update(meta_p, n_p, kpts, ident, score, frame_stream, state, mode=0, gate=0.7, kp_thr=0.3, min_common=3,
                  k2=None, new_thr=0.5, max_age=30):
    """``track_update_ref``'s signature on the device: outputs start as sentinels, the state is a
    copy, everything comes back to the host."""
    P, K = kpts.shape[:2]
    st = {k: v.clone().to(DEV) for k, v in state.items()}
    tid, hits, tident, tisc, status = _sentinels(P, len(frame_stream))
    ops.track_update(meta_p.to(DEV), torch.tensor([n_p], dtype=torch.int32, device=DEV), kpts.to(DEV), ident.to(DEV),
                     score.to(DEV), frame_stream.to(DEV), track_id=tid, track_hits=hits, track_ident=tident,
                     track_iscore=tisc, status=status, k2=TH.k2_for(K) if k2 is None else k2, mode=MODES[mode], gate=gate,
                     kp_thr=kp_thr, min_common=min_common, new_thr=new_thr, max_age=max_age, **st)
    return tid.cpu(), hits.cpu(), tident.cpu(), tisc.cpu(), status.cpu(), {k: v.cpu() for k, v in st.items()}


@pytest.mark.parametrize("name", sorted(TH.scenarios()))
def test_track_update_equals_the_restatement(name):
    got = TH.run(device_update, name)
    assert len(got) == len(TH.expected(name))
    for i, (want, have) in enumerate(zip(TH.expected(name), got)):
        assert TH.same(want, have), f"call {i}"


def test_two_runs_give_the_same_bits():
    S, K, kw, calls = TH.scenarios()["capacity"]
    a = device_update(*calls[0], TH.fresh_state(S, K), **kw)
    b = device_update(*calls[0], TH.fresh_state(S, K), **kw)
    assert TH.same(a, b) and TH.same(a, TH.expected("capacity")[0])


@pytest.mark.parametrize("name", ["walk_pose", "three_streams", "identity", "age_two"])
def test_one_call_equals_a_call_per_frame(name):
    """T frames in one call, or T calls that each track one of them (the others' stream is -1):
    the same outputs, the same state."""
    S, K, kw, calls = TH.scenarios()[name]
    meta_p, n_p, kpts, ident, score, fs = calls[0]
    whole = device_update(*calls[0], TH.fresh_state(S, K), **kw)
    assert TH.same(whole, TH.expected(name)[0])
    frame = meta_p.view(torch.int32)[:, 0]
    state = TH.fresh_state(S, K)
    outs = [torch.full_like(o, -5) for o in whole[:4]]
    status = torch.full_like(whole[4], -5)
    for b in range(len(fs)):
        only = torch.full_like(fs, -1)
        only[b] = fs[b]
        r = device_update(meta_p, n_p, kpts, ident, score, only, state, **kw)
        state = r[5]
        rows = (frame == b) & (torch.arange(len(frame)) < n_p)
        for o, part in zip(outs, r[:4]):
            o[rows] = part[rows]
        status[b] = r[4][b]
        others = torch.ones(len(fs), dtype=torch.bool)
        others[b] = False
        assert bool((r[4][others] == 0).all()) and bool((r[0][~rows] == -1).all())
    nobody = ~((frame >= 0) & (frame < len(fs)) & (torch.arange(len(frame)) < n_p))
    for o, w in zip(outs, whole[:4]):
        o[nobody] = w[nobody]
    assert TH.same((*outs, status, state), whole)


def test_streams_are_independent():
    S, K, kw, calls = TH.scenarios()["three_streams"]
    meta_p, n_p, kpts, ident, score, fs = calls[0]
    want = TH.expected("three_streams")[0]
    # the streams' labels permuted: the same outputs, the state permuted
    perm = torch.tensor([2, 0, 1])
    inside = (fs >= 0) & (fs < S)
    fs2 = torch.where(inside, perm[fs.clamp(0, S - 1).long()].int(), fs)
    got = device_update(meta_p, n_p, kpts, ident, score, fs2, TH.fresh_state(S, K), **kw)
    back = {k: v[perm] for k, v in got[5].items()}
    assert TH.same((*got[:5], back), want)
    # the slots of the other streams' persons shuffled among themselves: nothing changes for stream 0
    frame = meta_p.view(torch.int32)[:n_p, 0].long()
    mine = fs[frame] == 0
    rest = torch.nonzero(~mine).flatten()
    order = torch.arange(n_p)
    order[rest] = rest[torch.randperm(len(rest), generator=torch.Generator().manual_seed(3))]
    assert not torch.equal(order, torch.arange(n_p))
    sh = [t.clone() for t in (meta_p, kpts, ident, score)]
    for t, src in zip(sh, (meta_p, kpts, ident, score)):
        t[:n_p] = src[order]
    got = device_update(sh[0], n_p, sh[1], sh[2], sh[3], fs, TH.fresh_state(S, K), **kw)
    keep = torch.nonzero(mine).flatten()
    for g, w in zip(got[:4], want[:4]):
        assert torch.equal(TH.bits(g[keep]), TH.bits(w[keep]))
    assert all(torch.equal(TH.bits(got[5][k][0]), TH.bits(want[5][k][0])) for k in want[5])
    assert torch.equal(got[4][fs == 0], want[4][fs == 0])


def test_refusals_leave_outputs_and_state_untouched():
    """Every -EINVAL cause of include/prpe.h on real device buffers full of sentinels: the status is
    -22 and no byte of an output or of the state has changed."""
    P, B, S, K = 4, 2, 1, 17
    meta_p, n, kp, ident, score, fs = (t.to(DEV) if isinstance(t, torch.Tensor) else t
                                       for t in TH.call([[TH.person((0.0, 0.0, 20.0, 20.0))], []], max_p=P))
    n_p = torch.tensor([n], dtype=torch.int32, device=DEV)
    state = {"trk_meta": torch.full((S, 32, 8), 7.0, device=DEV), "trk_kpts": torch.full((S, 32, K, 3), 7.0, device=DEV),
             "trk_ident": torch.full((S, 32), 77, device=DEV, dtype=torch.int64),
             "trk_iscore": torch.full((S, 32), 7.0, device=DEV),
             "next_id": torch.full((S,), 77, device=DEV, dtype=torch.int32)}
    outs = _sentinels(P, B)
    written = list(state.values()) + list(outs)
    before = [t.clone() for t in written]
    ptrs = [t.data_ptr() for t in (meta_p, n_p, kp, ident, score, fs, *written)]
    for name, kw in sorted(TH.lib_refusals().items()):
        assert TH.lib_call(ptrs, **{"B": B, "S": S, "max_p": P, **kw}) == -22, name
    torch.cuda.synchronize()
    assert all(torch.equal(TH.bits(a), TH.bits(b)) for a, b in zip(written, before))
    assert TH.lib_call(ptrs, B=B, S=S, max_p=P) == 0          # the same call without any of the causes is taken
    torch.cuda.synchronize()
    assert outs[0].tolist()[1:] == [-1, -1, -1] and outs[4].tolist() == [0, 0]


# ---------------------------------------------------------------------------------- PersonTracker
@pytest.fixture(scope="module")
def model(state_dict):
    return CombinedModel(state_dict, device=DEV)


def _dets(frames_rows):
    d, c = TH.T._dets(frames_rows)
    return d.nan_to_num(0.0).to(DEV), c.to(DEV)


def _count_reads(monkeypatch):
    reads = []
    for name in ("cpu", "item", "tolist"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    return reads


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(TH.bits(a), TH.bits(b))


def test_person_tracker_equals_its_stages_run_apart(model, monkeypatch):
    """Two consecutive PersonRecognition outputs (64 x 96 frames, two cameras) through
    PersonTracker.update: the tracker's arrays are those of ops.track_update on a state of its
    own and of the restatement, PersonRecognition's arrays are handed through untouched and are the
    bits it gives without a tracker, and nothing is read back."""
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(41)).to(DEV)
    gallery = FaceGallery(dim=512, capacity=8, device=DEV)
    pose_kw = dict(max_per_frame=2, max_crops=4, box_scale=1.0)
    face_kw = dict(max_per_frame=3, max_crops=5, box_scale=1.0, threshold=0.0)
    pr = PersonRecognition(model, gallery, pose=pose_kw, faces=face_kw, kp_thr=0.0)
    ed, ec = _dets([[(10.0, 8.0, 40.0, 44.0, 0.9)], [(30.5, 10.25, 70.0, 50.0, 0.6)]])
    assert pr.faces.enrol_detections(x, ed, ec, [11, 13]) == []
    fd, fc = _dets([[(10.0, 8.0, 40.0, 44.0, 0.9)], [(30.5, 10.25, 70.0, 50.0, 0.6)]])
    none_d, none_c = _dets([[], []])
    pd1, pc1 = _dets([[(4.0, 2.0, 50.0, 62.0, 0.9), (50.0, 4.0, 118.0, 80.0, 0.8)], [(20.0, 5.0, 80.0, 60.0, 0.7)]])
    pd2, pc2 = _dets([[(6.0, 3.0, 52.0, 63.0, 0.9), (52.0, 5.0, 120.0, 81.0, 0.8)], [(22.0, 6.0, 82.0, 61.0, 0.7)]])
    plain1 = pr.from_detections(x, pd1, pc1, fd, fc)
    tracker = PersonTracker(pr, n_streams=2, new_thr=0.5, max_age=3)
    reads = _count_reads(monkeypatch)
    out1 = tracker.update(pr.from_detections(x, pd1, pc1, fd, fc))
    out2 = tracker.update(pr.from_detections(x, pd2, pc2, none_d, none_c))       # the faces are hidden
    assert reads == []
    monkeypatch.undo()
    for k in ("person_face", "person_ident", "person_score", "match_status"):
        assert _same(out1[k], plain1[k]), k
    for stage in ("pose", "faces"):
        for k in plain1[stage]:
            assert _same(out1[stage][k], plain1[stage][k]), (stage, k)
    assert set(out1) == set(plain1) | {"track_id", "track_hits", "track_ident", "track_ident_score", "track_status"}
    # the stages apart: ops.track_update on a fresh state of its own, and the restatement
    state = {k: v.to(DEV) for k, v in TH.fresh_state(2, 17).items()}
    host = TH.fresh_state(2, 17)
    fs = torch.tensor([0, 1], dtype=torch.int32)
    for out in (out1, out2):
        p = out["pose"]
        tid, hits, tident, tisc, status = _sentinels(4, 2)
        ops.track_update(p["crop_meta"], p["n_crops"], p["keypoints"], out["person_ident"], out["person_score"],
                         fs.to(DEV), track_id=tid, track_hits=hits, track_ident=tident, track_iscore=tisc,
                         status=status, k2=tracker.k2, mode="iou", gate=0.7, new_thr=0.5, max_age=3, **state)
        assert _same(out["track_id"], tid) and _same(out["track_hits"], hits) and _same(out["track_ident"], tident)
        assert _same(out["track_ident_score"], tisc) and _same(out["track_status"], status)
        ref = TH.track_update_ref(p["crop_meta"].cpu(), int(p["n_crops"]), p["keypoints"].cpu(), out["person_ident"].cpu(),
                                  out["person_score"].cpu(), fs, host, new_thr=0.5, max_age=3, k2=tracker.k2)
        host = ref[5]
        assert TH.same(ref, (tid.cpu(), hits.cpu(), tident.cpu(), tisc.cpu(), status.cpu(),
                             {k: v.cpu() for k, v in state.items()}))
    assert all(_same(tracker.state[k], state[k]) for k in state)
    # three persons, one id per camera and person, kept on the second frame; the names read on the
    # first frame outlive the second, on which no face was seen
    assert int(out1["pose"]["n_crops"]) == 3
    assert out1["track_id"].tolist() == [0, 1, 0, -1] == out2["track_id"].tolist()
    assert out2["track_hits"].tolist() == [2, 2, 2, 0]
    assert out2["person_ident"].tolist() == [-1] * 4
    named = out1["person_ident"][:3].tolist()
    assert any(v >= 0 for v in named) and out2["track_ident"][:3].tolist() == named == out1["track_ident"][:3].tolist()
    people = PersonTracker.results(out2)
    assert [[q["track_id"] for q in fr] for fr in people] == [[0, 1], [0]]
    assert [q["track_ident"] for fr in people for q in fr] == named and people[0][0]["ident"] == -1
    tracker.reset([1])
    out3 = tracker.update(pr.from_detections(x, pd2, pc2, none_d, none_c))
    assert out3["track_id"].tolist() == [0, 1, 0, -1] and out3["track_hits"].tolist() == [3, 3, 1, 0]


def test_person_tracker_full_path_reads_nothing_back(model, monkeypatch):
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(41)).to(DEV)
    gallery = FaceGallery(dim=512, capacity=4, device=DEV)
    gallery.add(torch.randn(2, 512, generator=torch.Generator().manual_seed(44)).to(DEV), [5, 6])
    branches = ("yolo_face", "yolo_person")
    saved = {b: getattr(model, b).yolo.head.stride for b in branches}
    for b in branches:
        getattr(model, b).yolo.head.stride = torch.tensor([8.0, 16.0, 32.0])
    try:
        pr = PersonRecognition(model, gallery, pose=dict(score_thr=0.0, max_per_frame=2),
                               faces=dict(score_thr=0.0, min_size=1.0, max_per_frame=2, threshold=-1.0))
        tracker = PersonTracker(pr, mode="pose", new_thr=0.0)
        want = pr(x)
        tracker(x)
        reads = _count_reads(monkeypatch)
        out = tracker(x, frame_stream=[0, 0])
        assert reads == []
        people = PersonTracker.results(out)
        assert reads == ["cpu"]                           # results() is the only read
        monkeypatch.undo()
    finally:
        for b, s in saved.items():
            getattr(model, b).yolo.head.stride = s
    for k in ("person_face", "person_ident", "person_score"):
        assert _same(out[k], want[k]), k                  # the tracker's presence changes nothing before it
    assert _same(out["pose"]["keypoints"], want["pose"]["keypoints"])
    n_p = int(out["pose"]["n_crops"])
    assert sum(len(p) for p in people) == n_p and out["track_status"].tolist() == [0, 0]
    tid = out["track_id"].cpu()
    assert bool((tid[:n_p] >= 0).all()) and bool((tid[n_p:] == -1).all())      # new_thr 0: everybody has a track
    assert all("track_id" in q and "track_ident_score" in q for fr in people for q in fr)
