"""GPU: per-face identification and the face-to-person match (csrc/roi.hip, prpe.faces) -- the
kernels against the restatements of tests/test_faces_host.py and against the top-down kernels they
generalise, and FaceCrops / PersonRecognition against the unfused routes through the public pieces.

Tolerances (none is taken from what the kernels give):
* roi_select: integer fields, window and score bit-exact; at 256 x 192 bit-equal to crop_select.
* roi_resize: into the top-down buffer's interior bit-equal to crop_resize / crop_resize_u8. At the
  other sizes the yardstick is F.affine_grid + F.grid_sample(bilinear, zeros, align_corners=False)
  in float64 on the CPU; its own fp32 noise e = max |yardstick - yardstick with its grid rounded to
  fp32| over the group's windows; the kernel is allowed 4 e (DESIGN.md §5b's convention).
  Everything outside the view keeps its sentinel, channel 3 and empty slots are exactly zero,
  y_amax has the bits of max|y| per slot.
* face_person_match: every output bit-equal to face_person_match_ref.
* FaceCrops / PersonRecognition: bit-identical to the unfused routes; identification scores of
  enrolled crops within 4 x the fp32 CPU normalise-and-dot's own distance from fp64 of 1.
"""
import pytest
import torch
import torch.nn.functional as F

import test_faces_host as FH
import test_topdown_host as T
from prpe import CombinedModel, FaceCrops, FaceGallery, FrameIngest, PersonRecognition, TopDownPose, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
H, W = 40, 56
STRIDE = [8.0, 16.0, 32.0]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _alloc(max_crops):
    return (torch.full((max_crops, 8), 7.0, device=DEV), torch.full((1,), -5, device=DEV, dtype=torch.int32),
            torch.full((1,), -5, device=DEV, dtype=torch.int32))


def _meta(rows, max_crops):
    """[(frame, (x0, y0, w, h)), ...] -> crop_meta [max_crops, 8] (host) as the select kernels lay it out."""
    meta = torch.zeros(max_crops, 8)
    ints = meta.view(torch.int32)
    ints[:, 0] = -1
    for s, (f, win) in enumerate(rows):
        ints[s, 0], ints[s, 1] = f, s
        meta[s, 2:6] = torch.stack([torch.as_tensor(v, dtype=torch.float32) for v in win])
        meta[s, 6] = 0.5
    return meta


# ---------------------------------------------------------------------------------- roi_select
def _random_dets():
    g = torch.Generator().manual_seed(5)
    B, max_det = 5, 8
    xy = torch.rand(B, max_det, 2, generator=g) * 100
    wh = torch.rand(B, max_det, 2, generator=g) * 60 + 10.0
    score = torch.sort(torch.rand(B, max_det, generator=g) * 0.7 + 0.3, dim=1, descending=True)[0]
    dets = torch.cat([xy, xy + wh, score[..., None], torch.zeros(B, max_det, 1)], 2)
    dets[3, 1, 0] = NAN                               # skipped, and uses up one of frame 3's two
    return dets, torch.tensor([3, 0, -1, 7, 1], dtype=torch.int32)


def _select_cases():
    """name -> (dets, counts, kwargs): tests/test_topdown_host.py's edge cases (both thresholds at
    equality, a negative count at frame 280 of 300, overflow in the second trip of the 256-frame
    scan, ...) and a random list at three capacities (overflow, exactly the list, room to spare)."""
    cases = {k: v[:3] for k, v in T.select_edge_cases().items()}
    dets, counts = _random_dets()
    kw = dict(score_thr=0.25, max_per_frame=2, min_size=4.0, box_scale=(1.7, 2.3), pad=1.25)
    for cap in (3, 4, 9):
        cases[f"random_{cap}"] = (dets, counts, dict(kw, max_crops=cap))
    # the aspect test at equality: a 30 x 30 box at 112 x 112 and a 30 x 20 box at 8 x 12 (a = 1.5)
    # take the else branch, which leaves both sides
    d, c = T._dets([[(10.0, 20.0, 40.0, 50.0, 0.9), (0.0, 0.0, 30.0, 20.0, 0.8)]])
    cases["square"] = (d, c, dict(pad=1.25, max_crops=4))
    return cases


def _roi_select(dets, counts, out_hw, max_crops=8, **kw):
    meta, n, st = _alloc(max_crops)
    ops.roi_select(dets.to(DEV), counts.to(DEV), (240, 320), out_hw, crop_meta=meta, n_crops=n, status=st, **kw)
    return meta.cpu(), int(n), int(st)


@pytest.mark.parametrize("name", sorted(_select_cases()))
def test_roi_select_at_256x192_has_crop_select_bits(name):
    dets, counts, kw = _select_cases()[name]
    kw = dict(kw)
    max_crops = kw.pop("max_crops", 8)
    want, n_w, st_w = _alloc(max_crops)
    ops.crop_select(dets.to(DEV), counts.to(DEV), (240, 320), crop_meta=want, n_crops=n_w, status=st_w, **kw)
    meta, n, st = _roi_select(dets, counts, (256, 192), max_crops, **kw)
    assert (n, st) == (int(n_w), int(st_w))
    assert torch.equal(_bits(meta), _bits(want.cpu()))
    if name == "random_3":
        assert (n, st) == (3, 3)                      # a negative count and an overflow past max_crops
    if name == "late_negative_count":
        assert (n, st) == (299, 1)


@pytest.mark.parametrize("out_hw", [(112, 112), (8, 12)])
@pytest.mark.parametrize("name", ["random_3", "random_9", "square", "aspect", "min_size", "prefix", "nonfinite",
                                  "late_negative_count", "late_overflow"])
def test_roi_select_matches_the_restatement_bit_for_bit(name, out_hw):
    dets, counts, kw = _select_cases()[name]
    ref, n_ref, st_ref = FH.roi_select_ref(dets, counts, out_hw, **kw)
    kw = dict(kw)
    meta, n, st = _roi_select(dets, counts, out_hw, kw.pop("max_crops", 8), **kw)
    assert (n, st) == (n_ref, st_ref)
    assert torch.equal(_bits(meta), _bits(ref))
    if name == "square":                              # the box at equality keeps both sides (times pad)
        s = 0 if out_hw == (112, 112) else 1
        assert n_ref == 2 and [float(v) for v in ref[s, 4:6]] == ([37.5, 37.5] if s == 0 else [37.5, 25.0])


# ---------------------------------------------------------------------------------- roi_resize
CONST = 0.7


def _frames():
    g = torch.Generator().manual_seed(7)
    big = torch.rand(3, 3, 48, 64, generator=g)
    big[2] = CONST
    return big


def _windows(out_hw):
    """(the windows the yardstick is held to, the slots that must come out as zeros)."""
    inside = (12.3, 6.4, 30.5, 24.25)                 # a window need not have the output's aspect
    good = [(0, inside),                              # wholly inside
            (1, FH.roi_window_ref(2, 1, 54, 39, 1.25, out_hw)),        # the box's own window: across the frame's edges
            (1, (-3.5, 2.25, 30.0, 20.0)), (0, (30.5, -4.0, 30.0, 20.0)),      # across the left / top edge only
            (1, (40.25, 20.5, 30.0, 30.0)),           # across the right and bottom edges
            (0, (-45.0, -35.0, 150.0, 112.5)),        # larger than the frame
            (1, (29.5, 19.5, 5.0, 5.0)),              # 4 x 4 pixels and a margin: heavy magnification
            (0, (0.0, 0.0, float(W), float(H))),      # exactly the frame
            (2, inside)]                              # the constant frame, every tap inside
    zero = [(-1, (5.0, 5.0, 20.0, 20.0)),             # no frame
            (3, (5.0, 5.0, 20.0, 20.0)),              # frame index B
            (0, (NAN, 5.0, 20.0, 20.0)), (1, (5.0, 5.0, INF, 20.0)), (0, (5.0, -INF, 20.0, INF)),
            (1, (5.0, 5.0, 20.0, NAN)),
            (0, (200.0, 150.0, 10.0, 10.0)),          # a filled slot wholly outside the frame
            (1, (-300.0, -300.0, 100.0, 100.0))]
    return good, zero


def _resize(out_hw, u8=None, y_amax=True, **kw):
    """One launch into a view inside a sentinel-filled buffer: (outer buffer, amax, meta, n) on the host."""
    oh, ow = out_hw
    good, zero = _windows(out_hw)
    rows = good + zero
    S = len(rows) + 2                                 # two slots at or past n_crops ...
    meta = _meta(rows, S)
    meta.view(torch.int32)[len(rows), 0] = 0          # ... one of them with a stale, valid-looking row
    meta[len(rows), 2:6] = torch.tensor([5.0, 5.0, 20.0, 20.0])
    outer = torch.full((S + 1, oh + 3, ow + 5, 4), 7.0, device=DEV)
    y = outer[:S, 1:1 + oh, 2:2 + ow, :]
    amax = torch.zeros(S, device=DEV) if y_amax else None
    n = torch.tensor([len(rows)], device=DEV, dtype=torch.int32)
    big = _frames()
    if u8 is None:
        frames = big.to(DEV)[:, :, 4:4 + H, 5:5 + W]  # a non-contiguous slice
        assert not frames.is_contiguous()
        ops.roi_resize(frames, meta.to(DEV), n, y, y_amax=amax)
    else:
        ops.roi_resize_u8(u8, meta.to(DEV), n, y, y_amax=amax, **kw)
    return outer.cpu(), None if amax is None else amax.cpu(), meta, len(good), len(rows)


SIZES = [(112, 112), (8, 12), (1, 1), (11, 130)]      # 130 columns: the column loop's second trip; 11 rows: a ragged block


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def resized(request):
    return (request.param, *_resize(request.param))


def test_roi_resize_against_cpu_grid_sample(resized):
    out_hw, outer, _, meta, n_good, _ = resized
    oh, ow = out_hw
    frames64 = _frames()[:, :, 4:4 + H, 5:5 + W].double()
    fr = meta.view(torch.int32)[:, 0]
    exact = [FH.roi_resize_ref(frames64, int(fr[s]), meta[s, 2:6], out_hw) for s in range(n_good)]
    noise = max(float((FH.roi_resize_ref(frames64, int(fr[s]), meta[s, 2:6], out_hw, True) - exact[s]).abs().max())
                for s in range(n_good))
    got = outer[:, 1:1 + oh, 2:2 + ow, :3]
    errs = [float((got[s].permute(2, 0, 1).double() - exact[s]).abs().max()) for s in range(n_good)]
    print(f"roi_resize {oh}x{ow}: yardstick fp32 noise {noise:.3e}, bound {4 * noise:.3e}, kernel max|d| per crop "
          + " ".join(f"{e:.3e}" for e in errs))
    assert 0.0 < noise < 1e-4
    assert max(errs) <= 4 * noise
    assert all(float(e.abs().max()) > 0.2 for e in exact)     # not vacuous: the crops hold the image
    assert bool((got[n_good - 1] == torch.tensor(CONST)).all())      # the constant frame: the constant exactly


def test_roi_resize_touches_only_the_view_and_clears_what_is_empty(resized):
    out_hw, outer, amax, meta, n_good, n_rows = resized
    oh, ow = out_hw
    S = outer.shape[0] - 1
    inner = torch.zeros_like(outer, dtype=torch.bool)
    inner[:S, 1:1 + oh, 2:2 + ow, :] = True
    assert bool((outer[~inner] == 7.0).all())         # the border, the extra slot: the sentinel
    y = outer[:S, 1:1 + oh, 2:2 + ow, :]
    assert float(y[..., 3].abs().max()) == 0.0        # channel 3
    assert float(y[n_good:].abs().max()) == 0.0       # no frame, frame B, NaN / inf windows, outside, past n_crops
    assert all(float(y[s].abs().max()) > 0.0 for s in range(n_good))
    want = y.abs().amax(dim=(1, 2, 3))
    assert torch.equal(_bits(amax), _bits(want)) and float(amax[n_good:].abs().max()) == 0.0
    assert float(amax[:n_good].min()) > 0.0


def test_roi_resize_without_amax_and_with_a_raised_slot():
    """y_amax is optional, and a slot that already holds more keeps it (the kernel only raises)."""
    out_hw = (8, 12)
    ref, amax, meta, n_good, n_rows = _resize(out_hw)
    got, none, *_ = _resize(out_hw, y_amax=False)
    assert none is None and torch.equal(_bits(got), _bits(ref))
    S = meta.shape[0]
    y = torch.zeros(S, 8, 12, 4, device=DEV)
    slots = torch.zeros(S, device=DEV)
    slots[0], slots[n_good] = 5.0, 3.0
    ops.roi_resize(_frames().to(DEV)[:, :, 4:4 + H, 5:5 + W], meta.to(DEV),
                   torch.tensor([n_rows], device=DEV, dtype=torch.int32), y, y_amax=slots)
    want = amax.clone()
    want[0], want[n_good] = 5.0, 3.0
    assert torch.equal(_bits(slots.cpu()), _bits(want))


def _u8_frames():
    big = (_frames() * 255).round().to(torch.uint8)
    big[2] = 179
    return big


@pytest.mark.parametrize("out_hw", [(112, 112), (11, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_roi_resize_u8_has_the_bits_of_the_float_route(out_hw):
    big = _u8_frames().to(DEV)
    u8 = big[:, :, 4:4 + H, 5:5 + W].permute(0, 2, 3, 1)      # NCHW slice seen as NHWC
    assert not u8.is_contiguous()
    oh, ow = out_hw
    good, zero = _windows(out_hw)
    rows = good + zero
    S = len(rows) + 1
    meta = _meta(rows, S).to(DEV)
    n = torch.tensor([len(rows)], device=DEV, dtype=torch.int32)

    def run(fn, frames, **kw):
        y, amax = torch.full((S, oh, ow, 4), 7.0, device=DEV), torch.zeros(S, device=DEV)
        fn(frames, meta, n, y, y_amax=amax, **kw)
        return y.cpu(), amax.cpu()
    ref, ref_amax = run(ops.roi_resize, big[:, :, 4:4 + H, 5:5 + W].float())
    got, amax = run(ops.roi_resize_u8, u8)
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(_bits(amax), _bits(ref_amax))
    assert float(ref[:len(good)].abs().max()) > 100.0 and float(ref[len(good):].abs().max()) == 0.0
    got, amax = run(ops.roi_resize_u8, u8.flip(3), swap_rb=True)       # BGR on channel-flipped frames
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(_bits(amax), _bits(ref_amax))
    # the affine: raw * a + b on every pixel of a filled slot (taps outside the frame are raw 0),
    # empty slots exact zeros, y_amax the maximum of what was written
    ing = FrameIngest(norm="imagenet")
    got, amax = run(ops.roi_resize_u8, u8, a=ing.a, b=ing.b)
    filled = torch.tensor([0 <= f < 3 for f, _ in rows] + [False])
    want = torch.zeros_like(ref)
    want[filled, :, :, :3] = ref[filled, :, :, :3] * torch.tensor(ing.a) + torch.tensor(ing.b)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(amax), _bits(want.abs().amax(dim=(1, 2, 3))))
    assert float(amax[len(good) + 6]) == max(abs(v) for v in ing.b)    # wholly outside the frame: b everywhere


def test_roi_resize_into_the_topdown_buffer_has_crop_resize_bits():
    """y = the interior of the top-down crop buffer (256 x 192): the bits of prpe_crop_resize and
    of prpe_crop_resize_u8, over the whole buffer."""
    big, big8 = _frames().to(DEV), _u8_frames().to(DEV)
    frames = big[:, :, 4:4 + H, 5:5 + W]
    u8 = big8[:, :, 4:4 + H, 5:5 + W].permute(0, 2, 3, 1)
    wins = [(0, T.window_ref(20, 8, 34, 26, 1.25)), (1, T.window_ref(2, 1, 54, 39, 1.25)),
            (0, T.window_ref(-30, -20, 90, 70, 1.25)), (-1, (0.0, 0.0, 0.0, 0.0)),
            (1, T.window_ref(30, 20, 34, 24, 1.25)), (0, (0.0, 0.0, float(W), float(H))),
            (7, T.window_ref(20, 8, 34, 26, 1.25)), (2, T.window_ref(2, 1, 54, 39, 1.25))]
    S = len(wins) + 1
    meta = _meta(wins, S).to(DEV)
    n = torch.tensor([len(wins)], device=DEV, dtype=torch.int32)
    ing = FrameIngest(norm="imagenet")

    def buffers():
        a = torch.zeros(S, 260, 196, 4, device=DEV)
        a[:, 2:-2, 2:-2, :3] = 1.0                    # stale crops everywhere
        return a, a.clone()
    want, got = buffers()
    ops.crop_resize(frames, meta, n, want)
    ops.roi_resize(frames, meta, n, got[:, 2:-2, 2:-2, :])
    assert torch.equal(_bits(got), _bits(want)) and float(want[0].abs().max()) > 0.5
    want, got = buffers()
    ops.crop_resize_u8(u8, meta, n, want, a=ing.a, b=ing.b, swap_rb=True)
    ops.roi_resize_u8(u8, meta, n, got[:, 2:-2, 2:-2, :], a=ing.a, b=ing.b, swap_rb=True)
    assert torch.equal(_bits(got), _bits(want)) and float(want[0].abs().max()) > 0.5


def test_roi_wrappers_refuse_bad_buffers():
    meta, n, _ = _alloc(4)
    frames = torch.zeros(1, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="y must be"):
        ops.roi_resize(frames, meta, n, torch.zeros(3, 12, 12, 4, device=DEV))                    # a slot short
    with pytest.raises(ValueError, match="y must be"):
        ops.roi_resize(frames, meta, n, torch.zeros(4, 12, 12, 8, device=DEV)[..., ::2])          # channel stride 2
    with pytest.raises(ValueError, match="y must be"):
        ops.roi_resize(frames, meta, n, torch.zeros(4, 12, 12, 5, device=DEV)[..., 1:])           # unaligned
    with pytest.raises(ValueError, match="slots"):
        ops.roi_resize(frames, meta, n, torch.zeros(4, 12, 12, 4, device=DEV), y_amax=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="output size"):
        ops.roi_select(torch.zeros(1, 1, 6, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32), (8, 8),
                       (0, 12), crop_meta=meta, n_crops=n, status=n.clone())


# ---------------------------------------------------------------------------------- face_person_match
def _match(args, **kw):
    mp, n_p, kp, mf, n_f, ident, score, B = args
    P = mp.shape[0]
    out = dict(face_slot=torch.full((P,), 77, device=DEV, dtype=torch.int32),
               person_ident=torch.full((P,), 77, device=DEV, dtype=torch.int64),
               person_score=torch.full((P,), 77.0, device=DEV), status=torch.full((B,), 77, device=DEV, dtype=torch.int32))
    i32 = lambda v: torch.tensor([v], device=DEV, dtype=torch.int32)
    ops.face_person_match(mp.to(DEV), i32(n_p), kp.to(DEV), mf.to(DEV), i32(n_f), ident.to(DEV), score.to(DEV), B,
                          **out, **kw)
    return tuple(out[k].cpu() for k in ("face_slot", "person_ident", "person_score", "status"))


@pytest.mark.parametrize("name", sorted(FH.match_edge_cases()))
def test_face_person_match_equals_the_restatement(name):
    args, want_face, want_status = FH.match_edge_cases()[name]
    face, ident, score, status = _match(args)
    r_face, r_ident, r_score, r_status = FH.face_person_match_ref(*args)
    assert torch.equal(face, r_face) and torch.equal(ident, r_ident) and torch.equal(_bits(score), _bits(r_score))
    assert status.tolist() == r_status.tolist() == want_status
    if want_face is not None:
        assert face[:args[1]].tolist() == want_face
    again = _match(args)                              # no atomics: the same bits again
    assert all(torch.equal(a, b) for a, b in zip(again[:2], (face, ident))) and torch.equal(_bits(again[2]), _bits(score))


def test_face_person_match_threshold_and_head_count_arguments():
    """kp_thr and head_kpts reach the kernel: with head_kpts = 1 only the first keypoint counts, and
    a threshold above every score sends every person to the fallback point."""
    args, _, _ = FH.match_edge_cases()["edges"]
    for kw in (dict(head_kpts=1), dict(kp_thr=0.95), dict(kp_thr=0.0, head_kpts=FH.K)):
        got = _match(args, **kw)
        want = FH.face_person_match_ref(*args, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(_bits(got[2]), _bits(want[2]))
    no_faces = list(args)
    no_faces[4] = 0                                   # n_f = 0: nobody matched, whatever the face rows hold
    got = _match(tuple(no_faces))
    assert bool((got[0] == -1).all()) and bool((got[1] == -1).all()) and bool((got[2] == -INF).all())


# ---------------------------------------------------------------------------------- FaceCrops
@pytest.fixture(scope="module")
def model(state_dict):
    return CombinedModel(state_dict, device=DEV)


def _model_frames(n=2):
    return torch.rand(n, 3, 64, 96, generator=torch.Generator().manual_seed(41)).to(DEV)


BOX_A, BOX_B, BOX_C, BOX_D = (10.0, 8.0, 40.0, 44.0), (60.0, 30.0, 110.0, 70.0), (30.5, 10.25, 70.0, 50.0), \
    (2.0, 30.0, 26.0, 60.0)


def _dets(frames_rows):
    d, c = T._dets(frames_rows)
    return d.nan_to_num(0.0).to(DEV), c.to(DEV)


def _face_dets():
    """Two frames, three boxes that give crops (one of them leaves the frame) and one below min_size."""
    return _dets([[(*BOX_A, 0.9), (50.0, 50.0, 52.0, 53.0, 0.8), (*BOX_B, 0.7)], [(*BOX_C, 0.6)]])


KW = dict(max_per_frame=3, max_crops=5, box_scale=1.0)


def test_face_crops_equal_the_unfused_route(model):
    x = _model_frames()
    dets, counts = _face_dets()
    e = model.engine
    before = model.forward_all(x, face_stride=STRIDE, concurrent=False)
    out = FaceCrops(model, compact=False, **KW).from_detections(x, dets, counts)
    n = int(out["n_crops"])
    assert n == 3 and int(out["status"]) == 0
    ref, n_ref, _ = FH.roi_select_ref(dets.cpu(), counts.cpu(), (112, 112), max_per_frame=3, max_crops=5)
    assert torch.equal(_bits(out["crop_meta"].cpu()), _bits(ref))
    assert T._frames_rows(ref, n_ref) == [(0, 0), (0, 2), (1, 0)]
    emb, norms = out["embeddings"].clone(), out["norms"].clone()
    # the whole-frame forward after the crops: the bits it gave before, and neither stem buffer moved
    keys = {k: v.data_ptr() for k, v in e._aux.items() if isinstance(k, tuple) and k[0] in ("stem_buf", "face_stem_buf")}
    assert set(keys) == {("stem_buf", 2, 70, 104, 4), ("face_stem_buf", 5, 118, 120, 4)}
    after = model.forward_all(x, face_stride=STRIDE, concurrent=False)
    assert all(_same(after[k], before[k]) for k in before)
    # compact: the trunk on the first n slots only, the same bits; alternating with whole frames
    # and a list capacity that is not the batch size reallocates neither buffer
    out_c = FaceCrops(model, compact=True, **KW).from_detections(x, dets, counts)
    model.forward_all(x, face_stride=STRIDE, concurrent=False)
    out_2 = FaceCrops(model, compact=False, **KW).from_detections(x, dets, counts)
    assert {k: v.data_ptr() for k, v in e._aux.items()
            if isinstance(k, tuple) and k[0] in ("stem_buf", "face_stem_buf")} == keys
    for o in (out_c, out_2):
        assert _same(o["embeddings"], emb) and _same(o["norms"], norms)
    # slots at or past n: zero embedding, nobody, -inf
    assert float(emb[n:].abs().max()) == 0.0 and float(norms[n:].abs().max()) == 0.0
    assert bool((out["ident"] == -1).all()) and bool((out["score"] == -INF).all())
    assert bool(torch.isfinite(emb).all())
    assert bool(((emb[:n].norm(dim=1) - 1).abs() < 1e-5).all())
    # the unfused route: the kernel's crops read back, then the public pieces (the frames' trunk
    # with batch n fills its own stem buffer with the same values and the same max|x| slots)
    buf = e.face_stem_buf(5)
    assert float(buf[n:].abs().max()) == 0.0          # nothing stale in the empty slots
    inner = torch.zeros_like(buf, dtype=torch.bool)
    inner[:, 3:115, 3:115, :3] = True
    assert float(buf[~inner].abs().max()) == 0.0      # the border and channel 3 stay zero
    crops = buf[:n, 3:115, 3:115, :3].permute(0, 3, 1, 2).contiguous()
    assert float(crops.abs().max()) > 0.5
    want, want_norm = e.adaface(e.trunk(crops))
    assert _same(emb[:n], want) and _same(norms[:n], want_norm.view(n))


def test_face_crops_identify_enrolled_faces(model):
    x = _model_frames()
    dets, counts = _dets([[(*BOX_A, 0.9), (50.0, 50.0, 52.0, 53.0, 0.8), (*BOX_B, 0.7)], [(*BOX_C, 0.6), (*BOX_D, 0.5)]])
    labels = [2 ** 35 + 1, 2 ** 35 + 2, 2 ** 35 + 3, 99]
    gallery = FaceGallery(dim=512, capacity=8, device=DEV)
    faces = FaceCrops(model, gallery, threshold=0.0, **KW)
    # enrolment: one face per frame; the fourth frame's only box is below score_thr
    ex = torch.stack([x[0], x[0], x[1], x[1]])
    ed, ec = _dets([[(*BOX_A, 0.9), (*BOX_D, 0.3)], [(*BOX_B, 0.7)], [(*BOX_C, 0.6)], [(*BOX_D, 0.2)]])
    assert faces.enrol_detections(ex, ed, ec, labels) == [3] and len(gallery) == 3
    out = faces.from_detections(x, dets, counts)
    n = int(out["n_crops"])
    assert n == 4
    emb = out["embeddings"][:n].cpu()
    s64 = F.normalize(emb.double(), dim=1) @ F.normalize(emb[:3].double(), dim=1).t()
    s32 = F.normalize(emb, dim=1) @ F.normalize(emb[:3], dim=1).t()
    bound = 4 * float((s32.double() - s64).abs().max())
    other_best = float(s64[3].max())
    off = s64[:3].clone()
    off.fill_diagonal_(-1.0)
    print(f"face crops e2e: bound={bound:.3e} fourth crop's best={other_best:.6f} enrolled crops' closest pair={float(off.max()):.6f}")
    assert other_best < 1 - 4 * bound and float(off.max()) < 1 - 4 * bound     # the crops are distinct
    assert (out["score"][:3].cpu() - 1).abs().max() <= bound
    assert abs(float(out["score"][3]) - other_best) <= bound
    assert out["ident"][:3].tolist() == labels[:3] and int(out["ident"][4]) == -1 and float(out["score"][4]) == -INF
    faces.threshold = 0.5 * (other_best + 1.0)
    for compact in (False, True):
        faces.compact = compact
        got = faces.from_detections(x, dets, counts)
        assert got["ident"].tolist() == labels[:3] + [-1, -1]
        assert _same(got["score"], out["score"]) and _same(got["embeddings"], out["embeddings"])
    people = FaceCrops.results(got)
    assert [[f["ident"] for f in fr] for fr in people] == [labels[:2], [labels[2], -1]]
    assert people[0][1]["row"] == 2 and people[1][1]["slot"] == 3


def _strides(model, branches):
    saved = {b: getattr(model, b).yolo.head.stride for b in branches}
    for b in branches:
        getattr(model, b).yolo.head.stride = torch.tensor(STRIDE)
    return saved


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


def test_face_crops_from_frames_u8_equals_the_float_entry_point(model, monkeypatch):
    """Raw normalisation and a stretch to the source's own size: the ingest writes u8.float(), the
    boxes map back by the identity, and the uint8 crops have the float crops' bits."""
    g = torch.Generator().manual_seed(43)
    u8 = torch.randint(0, 256, (2, 64, 96, 3), generator=g, dtype=torch.uint8).to(DEV)
    ing = FrameIngest(size=(64, 96), mode="stretch", norm=((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))
    x = u8.permute(0, 3, 1, 2).float()
    saved = _strides(model, ("yolo_face",))
    try:
        faces = FaceCrops(model, score_thr=0.0, min_size=1.0, max_per_frame=2)
        want = faces(x)
        reads = _count_reads(monkeypatch)
        got = faces.from_frames_u8(u8, ing)
        assert reads == []                            # the live path reads nothing back
        monkeypatch.undo()
    finally:
        for b, s in saved.items():
            getattr(model, b).yolo.head.stride = s
    assert set(got) == set(want) == {"dets", "counts", "crop_meta", "n_crops", "status", "embeddings", "norms",
                                     "ident", "score"}
    n = int(got["n_crops"])
    counts = got["counts"].cpu()
    print(f"face crops u8: counts {counts.tolist()} n_crops {n}")
    assert bool((counts >= 0).all()) and 0 < n <= 4
    assert got["embeddings"].shape == (4, 512)
    for k in ("counts", "crop_meta", "n_crops", "status", "embeddings", "norms", "ident", "score"):
        assert _same(got[k], want[k]), k


# ---------------------------------------------------------------------------------- PersonRecognition
def _person_dets():
    return _dets([[(4.0, 2.0, 50.0, 62.0, 0.9), (50.0, 4.0, 118.0, 80.0, 0.8)], [(20.0, 5.0, 80.0, 60.0, 0.7)]])


def test_person_recognition_equals_its_stages_run_apart(model):
    x = _model_frames()
    gallery = FaceGallery(dim=512, capacity=8, device=DEV)
    fd, fc = _face_dets()
    pd, pc = _person_dets()
    pose_kw, face_kw = dict(max_per_frame=2, max_crops=4, box_scale=1.0), dict(KW, threshold=0.0)
    pr = PersonRecognition(model, gallery, pose=pose_kw, faces=face_kw, kp_thr=0.0)
    ex = torch.stack([x[0], x[0], x[1]])
    ed, ec = _dets([[(*BOX_A, 0.9)], [(*BOX_B, 0.7)], [(*BOX_C, 0.6)]])
    assert pr.faces.enrol_detections(ex, ed, ec, [11, 12, 13]) == []
    out = pr.from_detections(x, pd, pc, fd, fc)
    want_p = TopDownPose(model, **pose_kw).from_detections(x, pd, pc)
    want_f = FaceCrops(model, gallery, **face_kw).from_detections(x, fd, fc)
    for k in want_p:
        assert _same(out["pose"][k], want_p[k]), k
    for k in want_f:
        assert _same(out["faces"][k], want_f[k]), k
    assert int(want_p["n_crops"]) == 3 and want_f["ident"].tolist() == [11, 12, 13, -1, -1]
    P = 4
    bufs = dict(face_slot=torch.empty(P, device=DEV, dtype=torch.int32),
                person_ident=torch.empty(P, device=DEV, dtype=torch.int64),
                person_score=torch.empty(P, device=DEV), status=torch.empty(2, device=DEV, dtype=torch.int32))
    ops.face_person_match(want_p["crop_meta"], want_p["n_crops"], want_p["keypoints"], want_f["crop_meta"],
                          want_f["n_crops"], want_f["ident"], want_f["score"], 2, kp_thr=0.0, head_kpts=5, **bufs)
    assert torch.equal(out["person_face"], bufs["face_slot"]) and torch.equal(out["person_ident"], bufs["person_ident"])
    assert _same(out["person_score"], bufs["person_score"]) and torch.equal(out["match_status"], bufs["status"])
    # ... and the restatement says the same of these lists
    ref = FH.face_person_match_ref(want_p["crop_meta"].cpu(), int(want_p["n_crops"]), want_p["keypoints"].cpu(),
                                   want_f["crop_meta"].cpu(), int(want_f["n_crops"]), want_f["ident"].cpu(),
                                   want_f["score"].cpu(), 2, kp_thr=0.0, head_kpts=5)
    assert torch.equal(out["person_face"].cpu(), ref[0]) and torch.equal(out["person_ident"].cpu(), ref[1])
    assert out["match_status"].tolist() == [0, 0] and int(out["person_face"][3]) == -1
    # results() round-trips them
    people = PersonRecognition.results(out)
    assert [len(p) for p in people] == [2, 1]
    flat = [p for fr in people for p in fr]
    meta_f = want_f["crop_meta"].cpu()
    for s, p in enumerate(flat):
        fs = int(out["person_face"][s])
        assert p["ident"] == int(out["person_ident"][s]) and p["ident_score"] == float(out["person_score"][s])
        assert torch.equal(p["keypoints"], want_p["keypoints"][s].cpu())
        if fs < 0:
            assert p["face_box"] is None and p["ident"] == -1
        else:
            x0, y0, w, h = (float(v) for v in meta_f[fs, 2:6])
            assert p["face_box"] == [x0, y0, x0 + w, y0 + h] and p["ident"] == [11, 12, 13][fs]


def test_person_recognition_full_path_reads_nothing_back(model, monkeypatch):
    x = _model_frames()
    gallery = FaceGallery(dim=512, capacity=4, device=DEV)
    gallery.add(torch.randn(2, 512, generator=torch.Generator().manual_seed(44)).to(DEV), [5, 6])
    saved = _strides(model, ("yolo_face", "yolo_person"))
    try:
        pr = PersonRecognition(model, gallery, pose=dict(score_thr=0.0, max_per_frame=2),
                               faces=dict(score_thr=0.0, min_size=1.0, max_per_frame=2, threshold=-1.0))
        pr(x)                                         # builds the person head's weight packs (Engine.prepare's job)
        reads = _count_reads(monkeypatch)
        out = pr(x)
        assert reads == []
        people = PersonRecognition.results(out)
        assert reads == ["cpu"]                       # results() is the only read
        monkeypatch.undo()
    finally:
        for b, s in saved.items():
            getattr(model, b).yolo.head.stride = s
    n_p, n_f = int(out["pose"]["n_crops"]), int(out["faces"]["n_crops"])
    assert out["person_face"].shape == (4,) and out["match_status"].tolist() == [0, 0]
    assert sum(len(p) for p in people) == n_p
    face = out["person_face"].cpu()
    assert bool((face[n_p:] == -1).all()) and bool((face < n_f).all())
    hit = face[face >= 0]
    assert hit.numel() == hit.unique().numel()        # one-to-one
    fi = out["faces"]["ident"].cpu()
    assert all(int(out["person_ident"][s]) == int(fi[int(face[s])]) for s in range(4) if int(face[s]) >= 0)
    assert bool(torch.isfinite(out["pose"]["keypoints"]).all())
