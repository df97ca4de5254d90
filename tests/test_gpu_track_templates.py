"""GPU: track-level face templates (csrc/tracktemplate.hip, prpe.tracks) -- prpe_track_template_update
and prpe_track_template_assign against ``track_template_update_ref`` / ``track_template_assign_ref``
of tests/test_track_templates_host.py (which a second, separately written statement agrees with on
every scenario), the gallery search on the templates, and ``PersonTracker(templates=...)``.

Tolerance: none. The sums are integers, a query row is one fixed conversion of them, and the
scores are the gallery search's own bits: every state array and every output is compared by
equality after every call of every scenario. Outputs and, where "untouched" is claimed, state
arrays start full of sentinels. Shapes: D = 32 and 512, 1 and 3 streams, 129 persons in 130 slots
(the ballots of one trip of the person walk cross three 64-lane chunks) and, because the walk takes
256 slots per trip, 650 persons in 700 slots (``long_walk``: three trips, a track without
candidates in the first or in the middle trip, the 2^20 limit reached in the third); 64 face slots."""
import numpy as np
import pytest
import torch

import test_track_templates_host as H
import test_tracks_host as TH
from prpe import CombinedModel, FaceGallery, PersonRecognition, PersonTracker, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
WEIGHTS = {0: "norm", 1: "uniform"}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i32(v):
    return torch.tensor([int(v)], dtype=torch.int32, device=DEV)


def _call_tensors(c, stride=None):
    emb = _dev(c["emb"])
    if stride is not None:                               # rows `stride` apart, NaN between them
        buf = torch.full((emb.shape[0], stride), NAN, device=DEV)
        buf[:, :emb.shape[1]] = emb
        emb = buf[:, :emb.shape[1]]
    return {"meta_p": _dev(c["meta_p"]), "n_p": _i32(c["n_p"]), "track_id": _dev(c["track_id"]),
            "person_face": _dev(c["person_face"]), "emb": emb, "norms": _dev(c["norms"]), "n_f": _i32(c["n_f"]),
            "frame_stream": _dev(c["frame_stream"]), "trk_meta": _dev(c["trk_meta"])}


def device_update(c, state, max_q, stride=None, keep=None):
    """``track_template_update_ref``'s signature on the device: outputs start as sentinels, the
    state is a copy, everything comes back to the host. ``keep``: a dict that receives the device
    tensors (for an assign that follows)."""
    t = _call_tensors(c, stride)
    S, _, D = state["tmpl_sum"].shape
    st = {k: _dev(v.copy()) for k, v in state.items()}
    rows = torch.full((max_q,), 77, device=DEV, dtype=torch.int32)
    nd = torch.full((1,), 77, device=DEV, dtype=torch.int32)
    pos = torch.full((S, 32), 77, device=DEV, dtype=torch.int32)
    q = torch.full((max_q, D), 7.0, device=DEV)
    ops.track_template_update(t["meta_p"], t["n_p"], t["track_id"], t["person_face"], t["emb"], t["norms"], t["n_f"],
                              t["frame_stream"], t["trk_meta"], dirty_rows=rows, n_dirty=nd, dirty_pos=pos, queries=q,
                              weight=WEIGHTS[c["weight_mode"]], min_norm=c["min_norm"], **st)
    if keep is not None:
        keep.update(t, state=st, dirty_rows=rows, n_dirty=nd, dirty_pos=pos, queries=q)
    return {k: v.cpu().numpy() for k, v in st.items()}, rows.cpu().numpy(), nd.cpu().numpy(), pos.cpu().numpy(), q.cpu().numpy()


def device_assign(k, ident, score):
    """prpe_track_template_assign on what ``device_update`` kept: (state after, the three outputs)."""
    P = k["meta_p"].shape[0]
    ti = torch.full((P,), 77, device=DEV, dtype=torch.int64)
    ts = torch.full((P,), 7.0, device=DEV)
    tf = torch.full((P,), 77, device=DEV, dtype=torch.int32)
    st = k["state"]
    ops.track_template_assign(k["meta_p"], k["n_p"], k["track_id"], k["frame_stream"], k["trk_meta"], ident, score,
                              k["n_dirty"], k["dirty_rows"], k["dirty_pos"], tmpl_n=st["tmpl_n"], tmpl_ident=st["tmpl_ident"],
                              tmpl_score=st["tmpl_score"], template_ident=ti, template_score=ts, template_faces=tf)
    return {n: v.cpu().numpy() for n, v in st.items()}, ti.cpu().numpy(), ts.cpu().numpy(), tf.cpu().numpy()


def _same_assign(a, b):
    return all(H.same_arrays(a[0][k], b[0][k]) for k in H.STATE_KEYS) and all(H.same_arrays(x, y) for x, y in zip(a[1:], b[1:]))


# ---------------------------------------------------------------------------------- the update
@pytest.mark.parametrize("name", sorted(H.scenarios()))
def test_update_equals_the_restatement(name):
    got = H.run(device_update, name)
    assert len(got) == len(H.expected(name))
    for i, (want, have) in enumerate(zip(H.expected(name), got)):
        assert H.same(want, have), f"call {i}"


def test_two_runs_give_the_same_bits():
    S, D, max_q, state, calls = H.scenarios()["random_D512_S3"]
    a, b = device_update(calls[0], state, max_q), device_update(calls[0], state, max_q)
    assert H.same(a, b) and H.same(a, H.expected("random_D512_S3")[0])


@pytest.mark.parametrize("name", ["random_D32_S1", "skips_D512"])
def test_row_stride_with_nan_in_the_padding(name):
    S, D, max_q, state, calls = H.scenarios()[name]
    assert H.same(device_update(calls[0], state, max_q, stride=D + 8), H.expected(name)[0])


def test_one_call_equals_a_call_per_frame():
    """Five frames in one call, or five calls that each see one of them (the others' stream is
    -1): the same sums, counts and owners."""
    S, D, max_q, state, calls = H.scenarios()["five_frames"]
    whole = device_update(calls[0], state, max_q)
    assert H.same(whole, H.expected("five_frames")[0])
    assert whole[0]["tmpl_n"][0, 3:5].tolist() == [4, 4] and int(whole[0]["tmpl_n"][1, 0]) == 1
    fs = calls[0]["frame_stream"]
    for b in range(len(fs)):
        only = np.full_like(fs, -1)
        only[b] = fs[b]
        state = device_update({**calls[0], "frame_stream": only}, state, max_q)[0]
    assert all(H.same_arrays(state[k], whole[0][k]) for k in H.STATE_KEYS)


def test_slot_order_of_persons_and_faces_does_not_matter():
    """The person slots permuted, the face slots permuted (and person_face with them): every
    stream's state is the bits it was."""
    S, D, max_q, state, calls = H.scenarios()["random_D512_S3"]
    c = calls[0]
    rng = np.random.default_rng(4)
    n_p, n_f = c["n_p"], c["n_f"]
    po, fo = rng.permutation(n_p), rng.permutation(n_f)               # new slot i holds old slot po[i] / fo[i]
    sh = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    for k in ("meta_p", "track_id", "person_face"):
        sh[k][:n_p] = c[k][po]
    sh["emb"][:n_f], sh["norms"][:n_f] = c["emb"][fo], c["norms"][fo]
    where = np.argsort(fo)                                            # old face slot -> new face slot
    pf = sh["person_face"][:n_p]
    sh["person_face"][:n_p] = np.where((pf >= 0) & (pf < n_f), where[np.clip(pf, 0, n_f - 1)], pf)
    got = device_update(sh, state, max_q)
    want = H.expected("random_D512_S3")[0]
    assert all(H.same_arrays(got[0][k], want[0][k]) for k in H.STATE_KEYS)
    assert H.same_arrays(got[3], want[3]) and H.same_arrays(got[4], want[4])


def test_slot_reuse_inside_one_call_through_the_real_tracker():
    """max_age = 0. Call 1: track A (id 0) opens in slot 0 and takes a face. Call 2, frame 0: A is
    seen again with a face; frame 1: A is missed and freed, B (id 1) opens in A's slot with a face.
    A's face of call 2 is dropped (no slot holds id 0 after the call), B starts from zero."""
    D = 32
    emb, norms = H.unit_rows(3, D, 21), np.array([9.0, 10.0, 11.0], np.float32)
    box, far = (10.0, 10.0, 20.0, 20.0), (500.0, 500.0, 20.0, 20.0)
    trk = {k: v.to(DEV) for k, v in TH.fresh_state(1, 17).items()}
    tmpl = H.fresh_templates(1, D)
    seen = []
    for frames, faces in (([[TH.person(box)]], [0]), ([[TH.person(box)], [TH.person(far)]], [1, 2])):
        meta, n, kp, ident, score, fs = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in TH.call(frames))
        P = meta.shape[0]
        tid = torch.full((P,), 77, device=DEV, dtype=torch.int32)
        outs = [torch.empty(P, device=DEV, dtype=d) for d in (torch.int32, torch.int64, torch.float32)]
        ops.track_update(meta, _i32(n), kp, ident, score, fs, track_id=tid, track_hits=outs[0], track_ident=outs[1],
                         track_iscore=outs[2], status=torch.empty(len(frames), device=DEV, dtype=torch.int32),
                         k2=TH.K2_17, max_age=0, **trk)
        face = np.full(P, -1, np.int32)
        face[:n] = faces
        c = {"meta_p": meta.cpu().numpy(), "n_p": n, "track_id": tid.cpu().numpy(), "person_face": face, "emb": emb,
             "norms": norms, "n_f": 3, "frame_stream": fs.cpu().numpy(), "trk_meta": trk["trk_meta"].cpu().numpy(),
             "weight_mode": 0, "min_norm": 0.0}
        got = device_update(c, tmpl, 3)
        assert H.same(got, H.track_template_update_ref(c, tmpl, 3))
        tmpl = got[0]
        seen.append((c["track_id"][:n].tolist(), int(c["trk_meta"].view(np.int32)[0, 0, 0]), got))
    assert seen[0][:2] == ([0], 0) and seen[1][:2] == ([0, 1], 1)
    assert int(seen[0][2][0]["tmpl_n"][0, 0]) == 1 and int(seen[0][2][0]["tmpl_owner"][0, 0]) == 0
    st = seen[1][2][0]
    assert int(st["tmpl_owner"][0, 0]) == 1 and int(st["tmpl_n"][0, 0]) == 1
    assert st["tmpl_sum"][0, 0].tolist() == [H.term(norms[2], v) for v in emb[2]]
    assert seen[1][2][1].tolist() == [0, -1, -1] and int(seen[1][2][2][0]) == 1


# ---------------------------------------------------------------------------------- identification
@pytest.mark.parametrize("name", ["random_D32_S3", "random_D512_S1", "list_full", "long_walk"])
def test_assign_equals_the_restatement(name):
    """Any search result (here: numbers that name their row) into the state and out to 130 (700) person
    slots; the state holds a preset name per slot, which the slots that are in no list keep."""
    S, D, max_q, state, calls = H.scenarios()[name]
    state = H.copy_state(state)
    rng = np.random.default_rng(2)
    for i, c in enumerate(calls):
        state["tmpl_ident"][:] = 1000 + np.arange(S * 32).reshape(S, 32)
        state["tmpl_score"][:] = rng.random((S, 32)).astype(np.float32)
        ident = (5000 + np.arange(max_q)).astype(np.int64)
        score = rng.random(max_q).astype(np.float32)
        keep = {}
        up = device_update(c, state, max_q, keep=keep)
        want = H.track_template_assign_ref(c, up[0], ident, score, up[2], up[1], up[3])
        got = device_assign(keep, _dev(ident), _dev(score))
        assert _same_assign(want, got), f"call {i}"
        nd = int(up[2][0])
        named = got[0]["tmpl_ident"].reshape(-1)
        assert sorted(named[named >= 5000].tolist()) == list(range(5000, 5000 + nd)) and nd > 0
        state = got[0]


def test_templates_are_identified_by_the_gallery_search():
    """template_score and template_ident are, bit for bit, what gallery.identify returns on the
    restatement's query rows; a slot that is not dirty keeps its preset name; persons of dead
    tracks and untracked persons get (-1, -inf, 0); template_faces is tmpl_n."""
    D, thr = 512, 0.2
    emb, norms = H.unit_rows(6, D, 31), np.array([7.0, 8.0, 9.0, 10.0, 11.0, 12.0], np.float32)
    gallery = FaceGallery(dim=D, capacity=8, device=DEV)
    gallery.add(_dev(np.concatenate([emb[:2] + 0.03 * emb[2:4], H.unit_rows(3, D, 32)])), [70, 71, 72, 73, 74])
    ids = H.ids_with(2, {(0, 2): 4, (0, 3): 6, (1, 9): 6, (1, 10): 8})
    persons = [(0, 4, -1), (0, 4, 9), (0, -1, 0), (0, 6, 0), (1, 6, 1), (1, 500, 2), (0, 6, 0), (1, 8, 4), (2, 6, 3)]
    c = H.make_call(ids, persons, emb, norms, [0, 1, 5], max_p=12)
    state = H.fresh_templates(2, D)
    state["tmpl_owner"][0, 2], state["tmpl_n"][0, 2], state["tmpl_sum"][0, 2] = 4, 3, 777
    state["tmpl_ident"][0, 2], state["tmpl_score"][0, 2] = 42, 0.5
    keep = {}
    up = device_update(c, state, 6, keep=keep)
    ref = H.track_template_update_ref(c, state, 6)
    assert H.same(up, ref) and int(ref[2][0]) == 3
    q_ident, q_score = gallery.identify(_dev(ref[4]), thr)
    got = device_assign(keep, q_ident, q_score)
    qi, qs = q_ident.cpu().numpy(), q_score.cpu().numpy()
    assert _same_assign(H.track_template_assign_ref(c, up[0], qi, qs, up[2], up[1], up[3]), got)
    assert qi[:3].tolist() == [70, 71, -1] and bool(qs[0] > 0.9) and bool(qs[2] < thr)
    st, ti, ts, tf = got
    assert ti.tolist() == [42, 42, -1, 70, 71, -1, 70, -1, -1] + [-1] * 3
    assert tf.tolist() == [3, 3, 0, 2, 1, 0, 2, 1, 0] + [0] * 3
    assert H.same_arrays(ts[[3, 4, 7]], qs[:3]) and ts[[0, 2, 5]].tolist() == [0.5, -INF, -INF]
    assert st["tmpl_ident"][0, 2:4].tolist() == [42, 70] and st["tmpl_ident"][1, 9:11].tolist() == [71, -1]
    assert (st["tmpl_sum"][0, 2] == 777).all()


def _track_then_fuse(gallery_rows, faces, norms, thr=H.THRESHOLD):
    """One person per frame in one place, face k on frame k: the single faces identified, the
    persons tracked by the real prpe_track_update, the template summed, searched and assigned.
    Returns (track_ident, template_ident, template_faces) of the last frame's person."""
    D, n = faces.shape[1], len(faces)
    gallery = FaceGallery(dim=D, capacity=4, device=DEV)
    gallery.add(_dev(gallery_rows), [7, 9])
    f_ident, f_score = (t.cpu() for t in gallery.identify(_dev(faces), thr))
    frames = [[TH.person((10.0, 10.0, 40.0, 60.0), ident=int(f_ident[k]), iscore=float(f_score[k]))] for k in range(n)]
    meta, n_p, kp, ident, score, fs = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in TH.call(frames))
    P = meta.shape[0]
    trk = {k: v.to(DEV) for k, v in TH.fresh_state(1, 17).items()}
    tid, hits = (torch.empty(P, device=DEV, dtype=torch.int32) for _ in range(2))
    tident, tisc = torch.empty(P, device=DEV, dtype=torch.int64), torch.empty(P, device=DEV)
    ops.track_update(meta, _i32(n_p), kp, ident, score, fs, track_id=tid, track_hits=hits, track_ident=tident,
                     track_iscore=tisc, status=torch.empty(n, device=DEV, dtype=torch.int32), k2=TH.K2_17, **trk)
    assert tid[:n].tolist() == [0] * n
    face = np.full(P, -1, np.int32)
    face[:n] = np.arange(n)
    c = {"meta_p": meta.cpu().numpy(), "n_p": n_p, "track_id": tid.cpu().numpy(), "person_face": face, "emb": faces,
         "norms": norms, "n_f": n, "frame_stream": fs.cpu().numpy(), "trk_meta": trk["trk_meta"].cpu().numpy(),
         "weight_mode": 0, "min_norm": 0.0}
    keep = {}
    up = device_update(c, H.fresh_templates(1, D), n, keep=keep)
    assert H.same(up, H.track_template_update_ref(c, H.fresh_templates(1, D), n))
    _, ti, ts, tf = device_assign(keep, *gallery.identify(keep["queries"], thr))
    return f_ident.tolist(), int(tident[n - 1]), int(ti[n - 1]), int(tf[n - 1])


def test_fusion_names_a_track_that_no_single_frame_names():
    """Four faces whose single cosines are 0.45 against a threshold of 0.5, whose sum is parallel to
    the gallery row (cosine 1): the margins, 0.04 and 0.4 beyond an fp32 slack of 1e-3, are asserted
    in fp64 by test_track_templates_host.test_margins_of_the_fusion_scenarios."""
    single, track_ident, template_ident, faces = _track_then_fuse(*H.fusion_faces())
    assert single == [-1] * 4 and track_ident == -1
    assert template_ident == 7 and faces == 4


def test_fusion_outvotes_one_confident_false_accept():
    """Eight frames of label 7 at cosine 0.9 and one frame that is label 9's gallery row itself: the
    best single frame names the track 9, the template 7 (margins: the same host test)."""
    single, track_ident, template_ident, faces = _track_then_fuse(*H.outlier_faces())
    assert single == [7, 7, 7, 9, 7, 7, 7, 7, 7] and track_ident == 9
    assert template_ident == 7 and faces == 9


# ---------------------------------------------------------------------------------- refusals
def test_refusals_leave_outputs_and_state_untouched():
    """Every -EINVAL cause of include/prpe.h on real device buffers full of sentinels: the status is
    -22 and no byte of an output or of the state has changed."""
    P, B, S, D, Fc, Q = 4, 2, 1, 32, 4, 4
    c = H.make_call(H.ids_with(1, {(0, 0): 0}), [(0, 0, 0)], H.unit_rows(Fc, D, 1), [5.0] * Fc, [0, 0], max_p=P)
    t = _call_tensors(c)
    state = [torch.full((S, 32), 77, device=DEV, dtype=torch.int32), torch.full((S, 32, D), 77, device=DEV, dtype=torch.int64),
             torch.full((S, 32), 77, device=DEV, dtype=torch.int32), torch.full((S, 32), 77, device=DEV, dtype=torch.int64),
             torch.full((S, 32), 7.0, device=DEV)]
    lists = [torch.full((Q,), 77, device=DEV, dtype=torch.int32), torch.full((1,), 77, device=DEV, dtype=torch.int32),
             torch.full((S, 32), 77, device=DEV, dtype=torch.int32), torch.full((Q, D), 7.0, device=DEV)]
    outs = [torch.full((P,), 77, device=DEV, dtype=torch.int64), torch.full((P,), 7.0, device=DEV),
            torch.full((P,), 77, device=DEV, dtype=torch.int32)]
    ident, score = torch.full((Q,), 5, device=DEV, dtype=torch.int64), torch.full((Q,), 0.5, device=DEV)
    written = state + lists + outs
    before = [w.clone() for w in written]
    up = [t[k].data_ptr() for k in ("meta_p", "n_p", "track_id", "person_face", "emb", "norms", "n_f", "frame_stream",
                                    "trk_meta")] + [w.data_ptr() for w in state + lists]
    asg = [t[k].data_ptr() for k in ("meta_p", "n_p", "track_id", "frame_stream", "trk_meta")] + \
          [w.data_ptr() for w in (ident, score, lists[1], lists[0], lists[2], state[2], state[3], state[4], *outs)]
    for name, kw in sorted(H.update_refusals().items()):
        assert H.lib_update(up, **kw) == -22, name
    for name, kw in sorted(H.assign_refusals().items()):
        assert H.lib_assign(asg, **kw) == -22, name
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(written, before))
    state[0].fill_(-1), state[1].zero_(), state[2].zero_()
    assert H.lib_update(up) == 0 and H.lib_assign(asg) == 0       # the same calls without any of the causes are taken
    torch.cuda.synchronize()
    assert lists[1].tolist() == [1] and lists[0].tolist() == [0, -1, -1, -1] and outs[0].tolist() == [5, -1, -1, -1]
    assert outs[2].tolist() == [1, 0, 0, 0] and int(state[0][0, 0]) == 0


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


def _same_t(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(TH.bits(a), TH.bits(b))


def _call_of(out, fs, trk_meta, weight_mode=0):
    p, f = out["pose"], out["faces"]
    return {"meta_p": p["crop_meta"].cpu().numpy(), "n_p": int(p["n_crops"]), "track_id": out["track_id"].cpu().numpy(),
            "person_face": out["person_face"].cpu().numpy(), "emb": f["embeddings"].cpu().numpy(),
            "norms": f["norms"].cpu().numpy(), "n_f": int(f["n_crops"]), "frame_stream": np.asarray(fs, np.int32),
            "trk_meta": trk_meta.cpu().numpy(), "weight_mode": weight_mode, "min_norm": 0.0}


def test_person_tracker_with_templates(model, monkeypatch):
    """Two consecutive PersonRecognition outputs (64 x 96 frames, two cameras) through two trackers,
    one with templates: every key and state array the plain tracker has holds the same bits, the
    template state is the restatement's, nothing is read back; reset, templates_host, enrol_track."""
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(41)).to(DEV)
    gallery = FaceGallery(dim=512, capacity=8, device=DEV)
    pr = PersonRecognition(model, gallery, pose=dict(max_per_frame=2, max_crops=4, box_scale=1.0),
                           faces=dict(max_per_frame=3, max_crops=5, box_scale=1.0, threshold=0.0), kp_thr=0.0)
    fd, fc = _dets([[(10.0, 8.0, 40.0, 44.0, 0.9)], [(30.5, 10.25, 70.0, 50.0, 0.6)]])
    assert pr.faces.enrol_detections(x, fd, fc, [11, 13]) == []
    pd1, pc1 = _dets([[(4.0, 2.0, 50.0, 62.0, 0.9), (50.0, 4.0, 118.0, 80.0, 0.8)], [(20.0, 5.0, 80.0, 60.0, 0.7)]])
    pd2, pc2 = _dets([[(6.0, 3.0, 52.0, 63.0, 0.9), (52.0, 5.0, 120.0, 81.0, 0.8)], [(22.0, 6.0, 82.0, 61.0, 0.7)]])
    outs = [pr.from_detections(x, pd1, pc1, fd, fc), pr.from_detections(x, pd2, pc2, fd, fc)]
    kw = dict(n_streams=2, new_thr=0.5, max_age=3)
    plain, fused = PersonTracker(pr, **kw), PersonTracker(pr, templates="norm", **kw)
    new = {"template_ident", "template_score", "template_faces"}
    host = H.fresh_templates(2, 512)
    reads = _count_reads(monkeypatch)
    got = [(plain.update(o), fused.update(o)) for o in outs]
    assert reads == []
    monkeypatch.undo()
    for a, b in got:
        assert not new & set(a) and set(b) == set(a) | new
        for k, v in a.items():
            if isinstance(v, dict):
                assert all(_same_t(v[n], b[k][n]) for n in v), k
            else:
                assert _same_t(v, b[k]), k
    assert all(_same_t(plain.state[k], fused.state[k]) for k in plain.state) and plain.template_state is None
    # the template state against the restatement, call by call on the tracker's own inputs
    trk = {k: v.to(DEV) for k, v in TH.fresh_state(2, 17).items()}
    for (_, b) in got:
        p = b["pose"]
        tmp = [torch.empty(4, device=DEV, dtype=d) for d in (torch.int32, torch.int32, torch.int64, torch.float32)]
        ops.track_update(p["crop_meta"], p["n_crops"], p["keypoints"], b["person_ident"], b["person_score"],
                         torch.tensor([0, 1], dtype=torch.int32, device=DEV), track_id=tmp[0], track_hits=tmp[1],
                         track_ident=tmp[2], track_iscore=tmp[3], status=torch.empty(2, device=DEV, dtype=torch.int32),
                         k2=fused.k2, mode="iou", gate=0.7, new_thr=0.5, max_age=3, **trk)
        c = _call_of(b, [0, 1], trk["trk_meta"])
        ref = H.track_template_update_ref(c, host, 5)
        qi, qs = gallery.identify(_dev(ref[4]), 0.0)
        asg = H.track_template_assign_ref(c, ref[0], qi.cpu().numpy(), qs.cpu().numpy(), ref[2], ref[1], ref[3])
        host = asg[0]
        assert H.same_arrays(b["template_ident"].cpu().numpy(), asg[1])
        assert H.same_arrays(b["template_score"].cpu().numpy(), asg[2])
        assert H.same_arrays(b["template_faces"].cpu().numpy(), asg[3])
    assert all(H.same_arrays(fused.template_state[k].cpu().numpy(), host[k]) for k in H.STATE_KEYS)
    faces = got[1][1]["template_faces"].tolist()
    face = got[1][1]["person_face"].tolist()
    assert max(faces) == 2 and faces[3] == 0 and max(face) >= 0
    # results(): one read, the three fields per person
    reads = _count_reads(monkeypatch)
    people = PersonTracker.results(got[1][1])
    assert reads == ["cpu"]
    monkeypatch.undo()
    flat = [q for fr in people for q in fr]
    assert [q["template_faces"] for q in flat] == faces[:3] and [q["template_ident"] for q in flat] == asg[1][:3].tolist()
    # templates_host, enrol_track, reset
    listed = fused.templates_host()
    assert [[t["track_id"] for t in s] for s in listed] == [[0, 1], [0]]
    assert [t["faces"] for s in listed for t in s] == [int(host["tmpl_n"][s, j]) for s, j in ((0, 0), (0, 1), (1, 0))]
    s, j = next((s, j) for s, j in ((0, 0), (0, 1), (1, 0)) if host["tmpl_n"][s, j] > 0)
    size = len(gallery)
    row = torch.from_numpy((host["tmpl_sum"][s, j].astype(np.float64) * 2.0 ** -24).astype(np.float32)).to(DEV)[None]
    want_rows, want_norms = torch.zeros(1, 512, device=DEV), torch.zeros(1, device=DEV)
    ops.gallery_enrol(row, want_rows, want_norms)
    assert fused.enrol_track(s, int(host["tmpl_owner"][s, j]), 55) == (size, size + 1) and len(gallery) == size + 1
    assert _same_t(gallery.rows[size], want_rows[0]) and int(gallery.labels[size]) == 55
    with pytest.raises(ValueError, match="not live"):
        fused.enrol_track(0, 31, 56)
    fused.reset([1])
    after = {k: v.cpu().numpy() for k, v in fused.template_state.items()}
    fresh = H.fresh_templates(2, 512)
    assert all(H.same_arrays(after[k][1], fresh[k][1]) and H.same_arrays(after[k][0], host[k][0]) for k in H.STATE_KEYS)
    assert fused.templates_host()[1] == [] and len(fused.templates_host()[0]) == 2


def test_an_empty_gallery_leaves_every_template_unnamed(model):
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(41)).to(DEV)
    pr = PersonRecognition(model, FaceGallery(dim=512, capacity=2, device=DEV),
                           pose=dict(max_per_frame=2, max_crops=4, box_scale=1.0),
                           faces=dict(max_per_frame=3, max_crops=5, box_scale=1.0, threshold=0.0), kp_thr=0.0)
    fd, fc = _dets([[(10.0, 8.0, 40.0, 44.0, 0.9)], [(30.5, 10.25, 70.0, 50.0, 0.6)]])
    pd1, pc1 = _dets([[(4.0, 2.0, 50.0, 62.0, 0.9), (50.0, 4.0, 118.0, 80.0, 0.8)], [(20.0, 5.0, 80.0, 60.0, 0.7)]])
    out = PersonTracker(pr, n_streams=2, templates="uniform").update(pr.from_detections(x, pd1, pc1, fd, fc))
    assert out["template_ident"].tolist() == [-1] * 4 and max(out["template_faces"].tolist()) == 1
    assert out["template_score"].tolist() == [-INF] * 4
