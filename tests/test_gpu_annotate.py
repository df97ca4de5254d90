"""GPU: annotated frames out (csrc/annotate.hip, prpe.annotate) -- prpe_annotate_nv12 and
prpe_annotate_u8 against ``annotate_nv12_ref`` / ``annotate_u8_ref`` of tests/test_annotate_host.py
(which a second, separately written statement agrees with), and ``Annotator`` against the ops.

Tolerance: none. After one fp32 rounding per coordinate everything is integers, so every comparison
is an equality over the WHOLE surface: the picture, the bytes between the picture and the pitch and
the rows below it, which start as a sentinel and must still hold it. The shapes are the smallest at
which the kernels take another path: an odd 70 x 45 (the chroma edge), exactly one tile and one
super-tile (sizes from prpe_annotate_geometry, not copied here), one pixel more than each, and
130 x 33."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_annotate_host as AH
from prpe import (Annotator, CombinedModel, FaceGallery, NV12Frames, PersonRecognition, PersonTracker, TopDownPose,
                  _lib, ops)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
SENT = 0xA5
TH, TW, SH, SW = ops.annotate_geometry()
SHAPES = [(45, 70), (TH, TW), (SH, SW), (TH + 1, TW + 1), (SH + 1, SW + 1), (33, 130)]


# ------------------------------------------------------------------ running a case on the device
def dev_lists(c):
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    persons = faces = None
    if len(c["meta_p"]):
        persons = (t(c["meta_p"]), torch.tensor([c["n_p"]], dtype=torch.int32, device=DEV), t(c["kpts"]), t(c["pcol"]))
    if len(c["meta_f"]):
        faces = (t(c["meta_f"]), torch.tensor([c["n_f"]], dtype=torch.int32, device=DEV), t(c["fmode"]), t(c["fcol"]))
    return persons, faces, t(c["palette"])


def kwargs(c):
    return dict(limbs=c["limbs"], box_t=c["box_t"], limb_r=c["limb_r"], kp_r=c["kp_r"], kp_thr=c["kp_thr"], cell=c["cell"],
                scale=(c["sx"], c["sy"]))


def work(c):
    return ops.annotate_workspaces(len(c["meta_p"]), len(c["meta_f"]), c["K"], len(c["limbs"]), DEV)


def nv12_surface(y, uv, pad=0, one=False, offset=0):
    """(NV12Frames, the surface(s) as device tensors, the same with ``y``, ``uv`` placed on the host)
    around sentinel bytes. ``one``: both planes are views of one surface; ``offset``: the luma plane
    starts that many bytes into its rows (an address that is not 8-byte aligned)."""
    B, H, W = y.shape
    Hc, Wc = uv.shape[1:3]
    up8 = lambda v: -(-v // 8) * 8
    # offset 0: pitches that are multiples of 8, as a decoder's are (the 8-byte paths); else the byte paths
    pitch = up8(2 * Wc + pad) if offset == 0 else 2 * Wc + pad
    if one:
        host = np.full((B, H + 3 + Hc + 1, pitch), SENT, np.uint8)
        host[:, :H, :W] = y
        host[:, H + 3:H + 3 + Hc, :2 * Wc] = uv.reshape(B, Hc, 2 * Wc)
        dev = torch.from_numpy(host).to(DEV)
        frames = NV12Frames.from_surface(dev, H, W, uv_row=H + 3)

        def expect(yo, uvo):
            e = host.copy()
            e[:, :H, :W] = yo
            e[:, H + 3:H + 3 + Hc, :2 * Wc] = uvo.reshape(B, Hc, 2 * Wc)
            return [e]
        return frames, [dev], expect
    hy = np.full((B, H + 2, up8(W + pad) if offset == 0 else W + pad + offset + 1), SENT, np.uint8)
    hu = np.full((B, Hc + 1, pitch), SENT, np.uint8)
    hy[:, :H, offset:offset + W] = y
    hu[:, :Hc, :2 * Wc] = uv.reshape(B, Hc, 2 * Wc)
    dy, du = torch.from_numpy(hy).to(DEV), torch.from_numpy(hu).to(DEV)
    frames = NV12Frames(dy[:, :H, offset:offset + W], du[:, :Hc, :2 * Wc].unflatten(2, (Wc, 2)))

    def expect(yo, uvo):
        ey, eu = hy.copy(), hu.copy()
        ey[:, :H, offset:offset + W] = yo
        eu[:, :Hc, :2 * Wc] = uvo.reshape(B, Hc, 2 * Wc)
        return [ey, eu]
    return frames, [dy, du], expect


def u8_surface(img, pad=0, planar=False):
    """(the [B, H, W, 3] view to paint, the buffer, expect(painted)) around sentinel bytes; ``planar``:
    an NCHW buffer seen through permute."""
    B, H, W, _ = img.shape
    if planar:
        host = np.full((B, 3, H + 1, W + pad), SENT, np.uint8)
        host[:, :, :H, :W] = img.transpose(0, 3, 1, 2)
        dev = torch.from_numpy(host).to(DEV)
        view = dev[:, :, :H, :W].permute(0, 2, 3, 1)

        def expect(out):
            e = host.copy()
            e[:, :, :H, :W] = out.transpose(0, 3, 1, 2)
            return e
        return view, dev, expect
    host = np.full((B, H + 1, W + pad, 3), SENT, np.uint8)
    host[:, :H, :W] = img
    dev = torch.from_numpy(host).to(DEV)

    def expect(out):
        e = host.copy()
        e[:, :H, :W] = out
        return e
    return dev[:, :H, :W], dev, expect


def check_case(c, seed=0, pad=6, one=False, offset=0, planar=False):
    """Both twins on one case: the whole surfaces equal the restatement's, the painted luma mask is
    the u8 twin's painted mask. Returns the mask."""
    y, uv, img = AH.surfaces(c["B"], c["H"], c["W"], seed)
    persons, faces, palette = dev_lists(c)
    table, means = work(c)
    frames, bufs, expect = nv12_surface(y, uv, pad, one, offset)
    ops.annotate_nv12(frames, palette, persons=persons, faces=faces, table=table, means=means, **kwargs(c))
    yo, uvo, m = AH.annotate_nv12_ref(c, y, uv)
    for got, want in zip(bufs, expect(yo, uvo)):
        assert np.array_equal(got.cpu().numpy(), want)
    view, buf, expect8 = u8_surface(img, pad, planar)
    ops.annotate_u8(view, palette, persons=persons, faces=faces, table=table, means=means, **kwargs(c))
    out, m8 = AH.annotate_u8_ref(c, img)
    got = buf.cpu().numpy()
    assert np.array_equal(got, expect8(out))
    assert np.array_equal(m, m8)
    return m


# ------------------------------------------------------------------ cases
def random_case(H, W, seed, B=3, n_persons=5, n_faces=4, **kw):
    """Persons and faces scattered so that windows, limbs and discs straddle tile, super-tile and
    frame edges, or lie wholly outside."""
    g = np.random.default_rng(seed)
    persons, faces = [], []
    for i in range(n_persons):
        cx, cy = g.uniform(-0.2 * W, 1.2 * W), g.uniform(-0.2 * H, 1.2 * H)
        w, h = g.uniform(4, 0.9 * W), g.uniform(4, 0.9 * H)
        kp = np.stack([g.uniform(cx - w / 2, cx + w / 2, 17), g.uniform(cy - h / 2, cy + h / 2, 17), g.uniform(0, 1, 17)], 1)
        persons.append((int(g.integers(0, B)), (cx - w / 2, cy - h / 2, w, h), kp, int(g.integers(0, 9))))
    for i in range(n_faces):
        w, h = g.uniform(1, 0.6 * W), g.uniform(1, 0.6 * H)
        faces.append((int(g.integers(0, B)), (g.uniform(-0.3 * W, W), g.uniform(-0.3 * H, H), w, h), int(g.integers(1, 3)),
                      int(g.integers(0, 9))))
    return AH.case(B, H, W, persons=persons, faces=faces, **kw)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_twins_equal_the_restatement(hw):
    H, W = hw
    m = check_case(random_case(H, W, seed=H * 1000 + W), seed=H + W, one=(H, W) == (45, 70))
    assert m.any() and not m.all()


def test_unaligned_planes_strided_views_and_scales():
    # a luma plane at an odd byte offset and an odd pitch's worth of padding: the byte paths; an NCHW
    # buffer for the u8 twin; sx, sy other than 1
    c = random_case(45, 70, seed=7, sx=1.5, sy=0.75, cell=2, limb_r=0, kp_r=1, box_t=1)
    assert check_case(c, seed=1, pad=4, offset=3, planar=True).any()
    c = random_case(TH + 1, TW + 1, seed=8, B=2, sx=0.5, sy=1.25, cell=64, limb_r=16, kp_r=16, box_t=16)
    assert check_case(c, seed=2, pad=2, offset=2).any()


def test_empty_lists_leave_the_surface_untouched():
    c = random_case(45, 70, seed=3, n_p=0, n_f=0)
    assert not check_case(c).any()
    c = random_case(45, 70, seed=3, n_p=-4, n_f=-1)
    assert not check_case(c).any()
    # no lists at all: legal, nothing runs
    y, uv, img = AH.surfaces(2, 9, 13, 0)
    frames, bufs, expect = nv12_surface(y, uv, 4)
    ops.annotate_nv12(frames, torch.zeros(2, 4, dtype=torch.uint8, device=DEV))
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(bufs, expect(y, uv)))
    # persons only (a pose-only caller), faces only
    c = random_case(45, 70, seed=4, n_faces=0)
    assert check_case(c).any()
    c = random_case(45, 70, seed=4, n_persons=0)
    assert check_case(c).any()


def _kp(pts, K=17):
    return AH._kp(pts, K)


def test_degenerate_and_extreme_primitives():
    H, W = TH + 1, TW + 1
    thr = np.float32(0.3)
    below = float(np.nextafter(thr, np.float32(0)))
    k = _kp({0: (10.0, 10.0, 1.0), 1: (10.0, 10.0, 1.0),             # L2 = 0
             2: (NAN, 5.0, 1.0), 3: (5.0, INF, 1.0), 4: (-INF, 5.0, 1.0),          # not finite
             5: (30.0, 30.0, NAN), 6: (40.0, 30.0, float(thr)), 7: (50.0, 30.0, below),     # scores
             8: (20479.0, 20.0, 1.0), 9: (20480.0, 40.0, 1.0), 10: (-4096.0, 50.0, 1.0), 11: (-4097.0, 60.0, 1.0),
             12: (3.0e38, 3.0e38, 1.0), 13: (W - 1.0, H - 1.0, 1.0), 14: (-200.0, -200.0, 1.0), 15: (W + 9.0, 32.0, 1.0),
             16: (0.0, 0.0, 1.0)})
    limbs = ((0, 1), (6, 8), (6, 9), (10, 13), (11, 13), (13, 14), (16, 13), (6, 7), (5, 6), (2, 0), (12, 0), (15, 13), (6, 15))
    persons = [(0, (5.0, 5.0, 30.0, 40.0), k, 0),
               (0, (20.0, 20.0, 3.0, 3.0), None, 1),                  # box_t larger than half the window
               (0, (NAN, 2.0, 5.0, 5.0), k, 2), (0, (2.0, 2.0, INF, 5.0), None, 2), (0, (2.0, 2.0, 3.0e38, 5.0), None, 2),
               (0, (-4096.0, -4096.0, 24575.0, 24575.0), None, 3),    # the largest window: its outline is outside
               (0, (-4096.0, 3.0, 24576.0, 9.0), None, 3),            # one past the limit: skipped
               (0, (-3.0, -3.0, 7.0, 7.0), None, 4), (0, (W - 3.0, H - 3.0, 50.0, 50.0), None, 5),
               (0, (10.0, 10.0, 0.0, 5.0), None, 6), (0, (10.0, 10.0, -4.0, 5.0), None, 6),      # empty windows
               (1, (W + 5.0, 2.0, 9.0, 9.0), k + np.float32(500.0), 1)]        # wholly outside
    for r in (0, 1, 16):
        c = AH.case(2, H, W, persons=persons, limbs=limbs, box_t=max(r, 1) if r < 16 else 16, limb_r=r, kp_r=r)
        assert check_case(c, seed=r).any()
    # stale rows past n, frame -1 and B
    stale = [(0, (4.0, 4.0, 20.0, 20.0), k, 0), (-1, (4.0, 4.0, 20.0, 20.0), k, 1), (2, (4.0, 4.0, 20.0, 20.0), k, 1),
             (1, (8.0, 8.0, 20.0, 20.0), k, 2), (1, (30.0, 8.0, 20.0, 20.0), k, 3)]
    fst = [(0, (3.0, 3.0, 9.0, 9.0), 1, 0), (-1, (3.0, 3.0, 9.0, 9.0), 2, 0), (2, (3.0, 3.0, 9.0, 9.0), 2, 0),
           (1, (3.0, 3.0, 9.0, 9.0), 2, 0), (1, (20.0, 3.0, 9.0, 9.0), 2, 0)]
    c = AH.case(2, 45, 70, persons=stale, faces=fst, n_p=4, n_f=4, max_p=7, max_f=6)
    assert check_case(c).any()
    c = AH.case(2, 45, 70, persons=stale, faces=fst, n_p=99, n_f=99, max_p=7, max_f=6)      # a count past the capacity
    assert check_case(c).any()


def test_more_primitives_on_one_tile_than_any_chunk():
    """32 persons with K = 64 and 32 limbs, all on one tile: 3104 primitives for lists of 256."""
    g = np.random.default_rng(11)
    K = 64
    limbs = tuple((int(a), int(b)) for a, b in g.integers(0, K, (32, 2)))
    persons = []
    for i in range(32):
        kp = np.stack([g.uniform(-4, TW + 4, K), g.uniform(-4, TH + 4, K), g.uniform(0.3, 1, K)], 1)
        persons.append((0, (g.uniform(0, 30), g.uniform(0, 30), g.uniform(5, 40), g.uniform(5, 40)), kp, i))
    c = AH.case(1, TH, TW, persons=persons, K=K, limbs=limbs, limb_r=0, kp_r=1, box_t=1,
                faces=[(0, (0.0, 0.0, float(TW), float(TH)), 1, 0)])
    m = check_case(c)
    assert m.all()                                          # the face under everything paints what is left
    # more owners than one chunk of the owner scan: 300 persons of one disc each
    persons = [(i % 2, (0.0, 0.0, 4.0, 4.0), _kp({0: (3.0 + (i * 7) % 60, 2.0 + (i * 13) % 40, 1.0)}), i) for i in range(300)]
    c = AH.case(2, 45, 70, persons=persons, limbs=(), box_t=0, kp_r=2,
                faces=[(i % 2, (float(i % 64), float(i % 40), 3.0, 3.0), 2, i) for i in range(270)])
    assert check_case(c).any()


def test_faces():
    H, W = 45, 70
    faces = [(0, (5.0, 5.0, 30.0, 30.0), 1, 0), (0, (20.0, 10.0, 30.0, 20.0), 2, 1), (0, (25.0, 15.0, 30.0, 25.0), 1, 0),
             (1, (-20.0, 10.0, 40.0, 30.0), 1, 0),                   # half off the frame
             (1, (50.0, 30.0, 40.0, 40.0), 1, 0),                    # off the far corner: the odd chroma edge
             (1, (33.0, 7.0, 1.0, 1.0), 1, 0), (1, (40.0, 8.0, 1.0, 1.0), 2, 2),      # windows of one pixel
             (2, (-100.0, -100.0, 400.0, 400.0), 1, 0),              # a close-up: the block side grows past cell
             (0, (60.0, 2.0, 9.0, 9.0), 0, 0), (0, (60.0, 2.0, 9.0, 9.0), 3, 0), (0, (1.0, 36.0, 9.0, 9.0), 2, 10 ** 9),
             (0, (12.0, 36.0, 9.0, 9.0), 2, -3)]                      # modes that leave; colour index wrap
    for cell in (2, 8, 64):
        c = AH.case(3, H, W, faces=faces, cell=cell,
                    persons=[(0, (8.0, 8.0, 20.0, 20.0), _kp({0: (15.0, 15.0, 1.0), 1: (40.0, 30.0, 1.0)}), 7)])
        m = check_case(c, seed=cell, one=cell == 8)
        assert m[2].all() and not m[0].all()
    assert check_case(AH.case(3, SH + 1, SW + 1, faces=[(f, (b[0] * 2.0, b[1] * 2.0, b[2] * 2.0, b[3] * 2.0), md, col)
                                                          for f, b, md, col in faces])).any()


def test_priority_does_not_depend_on_the_other_layers_slot_order():
    """Person A in slot 0 and B in slot 1, or the other way round, with the faces' order reversed too:
    a disc still beats a limb beats a box beats a face whoever owns them, and only ties inside a layer
    follow the slots."""
    ka = _kp({5: (10.0, 10.0, 1.0), 6: (50.0, 30.0, 1.0)})
    kb = _kp({5: (50.0, 10.0, 1.0), 6: (10.0, 30.0, 1.0)})
    A_, B_ = (0, (5.0, 5.0, 50.0, 30.0), ka, 0), (0, (8.0, 8.0, 50.0, 30.0), kb, 1)
    f1, f2 = (0, (0.0, 0.0, 40.0, 40.0), 2, 2), (0, (20.0, 10.0, 45.0, 30.0), 1, 3)
    kw = dict(limbs=((5, 6),), limb_r=2, kp_r=4, box_t=3)
    outs = []
    for persons, faces in (((A_, B_), (f1, f2)), ((B_, A_), (f1, f2)), ((A_, B_), (f2, f1))):
        c = AH.case(1, 45, 70, persons=list(persons), faces=list(faces), **kw)
        check_case(c)
        outs.append(AH.keys_ref(c) >> 28)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])       # the layers do not move
    assert set(np.unique(outs[0])) == {0, 1, 2, 3, 4}


def test_two_runs_give_the_same_bytes():
    c = random_case(SH + 1, SW + 1, seed=21, n_persons=8, n_faces=6)
    y, uv, _ = AH.surfaces(c["B"], c["H"], c["W"], 3)
    persons, faces, palette = dev_lists(c)
    got = []
    for _ in range(2):
        table, means = work(c)
        frames, bufs, _e = nv12_surface(y, uv, 10)
        ops.annotate_nv12(frames, palette, persons=persons, faces=faces, table=table, means=means, **kwargs(c))
        got.append([b.cpu() for b in bufs] + [table.cpu(), means.cpu()])
    assert all(torch.equal(a, b) for a, b in zip(got[0][:2], got[1][:2]))


def test_refusals_leave_surfaces_and_workspaces_untouched():
    """Every -EINVAL cause on real device buffers full of sentinels: the status is -22 and no byte of
    a surface, the table or the means has changed; the same call without a cause is taken."""
    c = random_case(45, 70, seed=5, B=2, n_persons=4, n_faces=3)
    persons, faces, palette = dev_lists(c)
    B, H, W = 2, 45, 70
    surf = torch.full((B, H + 24, 72), SENT, dtype=torch.uint8, device=DEV)
    img = torch.full((B, H, W, 3), SENT, dtype=torch.uint8, device=DEV)
    table = torch.full((ops.annotate_table_bytes(4, 3, 17, 2),), SENT, dtype=torch.uint8, device=DEV)
    means = torch.full((3, 17, 17, 4), SENT, dtype=torch.uint8, device=DEV)
    written = [surf, img, table, means]
    before = [t.clone() for t in written]
    real = dict(crop_meta_p=persons[0].data_ptr(), n_p=persons[1].data_ptr(), keypoints=persons[2].data_ptr(),
                person_colour=persons[3].data_ptr(), crop_meta_f=faces[0].data_ptr(), n_f=faces[1].data_ptr(),
                face_mode=faces[2].data_ptr(), face_colour=faces[3].data_ptr(), palette=palette.data_ptr(),
                table=table.data_ptr(), means=means.data_ptr(), table_bytes=table.numel(), n_colours=len(c["palette"]))
    nv = dict(y=surf.data_ptr(), uv=surf.data_ptr() + H * 72, n=B, h=H, w=W, y_sn=surf.stride(0), y_sh=72,
              uv_sn=surf.stride(0), uv_sh=72)
    u8 = dict(ptr=img.data_ptr(), n=B, h=H, w=W, c=3, sn=img.stride(0), sh=img.stride(1), sw=3, sc=1)
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def args(**kw):
        bad = dict(kw)
        for k in ("palette", "means", "table"):          # a misaligned pointer, not the test's placeholder address
            if isinstance(bad.get(k), int):
                bad[k] = real[k] + (bad[k] - AH.P0)
        return AH.lib_args(**{**real, **bad})
    for call, good, surf_bad, base in ((L.prpe_annotate_nv12, AH.nv_surface, AH.NV_BAD, nv),
                                       (L.prpe_annotate_u8, AH.u8_surface, AH.U8_BAD, u8)):
        for kw in surf_bad:
            kw = {k: (base["uv"] + 1 if k == "uv" and v is not None else v) for k, v in kw.items()}
            assert call(C.byref(good(**{**base, **kw})), C.byref(args()), stream) == -22, kw
        for cause, kw in sorted(AH.lib_refusals().items()):
            assert call(C.byref(good(**base)), C.byref(args(**kw)), stream) == -22, cause
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(written, before))
    assert L.prpe_annotate_nv12(C.byref(AH.nv_surface(**nv)), C.byref(args()), stream) == 0
    assert L.prpe_annotate_u8(C.byref(AH.u8_surface(**u8)), C.byref(args()), stream) == 0
    torch.cuda.synchronize()
    assert not torch.equal(surf, before[0]) and not torch.equal(img, before[1])


# ------------------------------------------------------------------ Annotator
@pytest.fixture(scope="module")
def model(state_dict):
    return CombinedModel(state_dict, device=DEV)


def _dets(frames_rows):
    import test_gpu_tracks as GT
    return GT._dets(frames_rows)


def _count_reads(monkeypatch):
    import test_gpu_tracks as GT
    return GT._count_reads(monkeypatch)


def _case_of(out, persons, faces, palette, annot, B, H, W):
    """The restatement's inputs from the arrays an Annotator call handed to the ops."""
    h = lambda t: t.cpu().numpy()
    c = AH.case(B, H, W, limbs=annot.limbs, **{k: v for k, v in annot.kw.items()})
    c.update(meta_p=h(persons[0]), n_p=int(persons[1]), kpts=h(persons[2]), pcol=h(persons[3]), K=persons[2].shape[1],
             palette=h(palette))
    if faces is not None:
        c.update(meta_f=h(faces[0]), n_f=int(faces[1]), fmode=h(faces[2]), fcol=h(faces[3]))
    return c


def test_annotator_equals_the_ops_and_the_restatement(model, monkeypatch):
    """On the seeded model at the tracker tests' frame size: ``Annotator`` on a ``PersonTracker`` output
    equals ops.annotate_* on that output's arrays and the restatement, for both surfaces, and reads
    nothing back; with the gallery emptied, redact="unknown" pixelates every face; a pose-only output
    draws skeletons."""
    B, H, W = 2, 64, 96
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(41)).to(DEV)
    gallery = FaceGallery(dim=512, capacity=8, device=DEV)
    pr = PersonRecognition(model, gallery, pose=dict(max_per_frame=2, max_crops=4, box_scale=1.0),
                           faces=dict(max_per_frame=3, max_crops=5, box_scale=1.0, threshold=0.0), kp_thr=0.0)
    ed, ec = _dets([[(10.0, 8.0, 40.0, 44.0, 0.9)], [(30.5, 10.25, 70.0, 50.0, 0.6)]])
    assert pr.faces.enrol_detections(x, ed, ec, [11, 13]) == []
    fd, fc = _dets([[(10.0, 8.0, 40.0, 44.0, 0.9), (60.0, 20.0, 80.0, 40.0, 0.5)], [(30.5, 10.25, 70.0, 50.0, 0.6)]])
    pd, pc = _dets([[(4.0, 2.0, 50.0, 62.0, 0.9), (50.0, 4.0, 118.0, 80.0, 0.8)], [(20.0, 5.0, 80.0, 60.0, 0.7)]])
    tracker = PersonTracker(pr, n_streams=2, new_thr=0.5)
    out = tracker.update(pr.from_detections(x, pd, pc, fd, fc))
    y, uv, img = AH.surfaces(B, H, W, 9)
    annot = Annotator(colour_by="track", redact="unknown", kp_thr=0.0)
    frames, bufs, expect = nv12_surface(y, uv, 8, one=True)
    view, buf8, expect8 = u8_surface(img, 5)
    annot(frames, out)                                       # the caches fill: palettes and workspaces
    frames, bufs, expect = nv12_surface(y, uv, 8, one=True)
    reads = _count_reads(monkeypatch)
    annot(frames, out)
    annot(view, out)
    assert reads == []
    monkeypatch.undo()
    persons, faces = annot.lists(out)
    for surface, ref in ((frames, "nv12"), (view, "u8")):
        c = _case_of(out, persons, faces, annot.palette(surface), annot, B, H, W)
        table, means = work(c)
        if ref == "nv12":
            yo, uvo, m = AH.annotate_nv12_ref(c, y, uv)
            assert np.array_equal(bufs[0].cpu().numpy(), expect(yo, uvo)[0])
            f2, b2, _ = nv12_surface(y, uv, 8, one=True)
            ops.annotate_nv12(f2, annot.palette(surface), persons=persons, faces=faces, table=table, means=means,
                              limbs=annot.limbs, **annot.kw)
            assert torch.equal(b2[0], bufs[0])
        else:
            o8, m = AH.annotate_u8_ref(c, img)
            assert np.array_equal(buf8.cpu().numpy(), expect8(o8))
            v2, b2, _ = u8_surface(img, 5)
            ops.annotate_u8(v2, annot.palette(surface), persons=persons, faces=faces, table=table, means=means,
                            limbs=annot.limbs, **annot.kw)
            assert torch.equal(b2, buf8)
        assert m.any()
    # the gallery emptied: nobody is known, every face is pixelated
    gallery.reset()
    out2 = pr.from_detections(x, pd, pc, fd, fc)
    a2 = Annotator(colour_by="ident", redact="unknown", kp_thr=0.0)
    assert a2.lists(out2)[1][2].tolist() == [1] * 5
    view2, buf2, expect2 = u8_surface(img, 5)
    a2(view2, out2)
    c = _case_of(out2, *a2.lists(out2), a2.palette(view2), a2, B, H, W)
    o8, m = AH.annotate_u8_ref(c, img)
    assert np.array_equal(buf2.cpu().numpy(), expect2(o8))
    faces_only = AH.keys_ref(dict(c, n_p=0)) > 0
    assert faces_only.sum() > 0 and m[faces_only].all()
    # a pose-only output draws skeletons; coords_hw scales them onto a larger surface
    pose = TopDownPose(model, max_per_frame=2, max_crops=4, box_scale=1.0).from_detections(x, pd, pc)
    a3 = Annotator(colour_by="slot", kp_thr=0.0)
    y2, uv2, _ = AH.surfaces(B, 2 * H, 2 * W + 1, 10)
    f3, b3, e3 = nv12_surface(y2, uv2, 3)
    a3(f3, pose, coords_hw=(H, W))
    c = _case_of(pose, *a3.lists(pose), a3.palette(f3), a3, B, 2 * H, 2 * W + 1)
    c.update(sx=(2 * W + 1) / float(W), sy=2.0)
    yo, uvo, m = AH.annotate_nv12_ref(c, y2, uv2)
    assert m.any() and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(b3, e3(yo, uvo)))


def test_palette_helper_on_the_device_for_both_matrices_and_ranges():
    """A filled face through Annotator on NV12 surfaces of every matrix and range: the bytes painted
    are rgb_to_yuv's, and converting the frame back gives the colour within the helper's bound."""
    out = {"pose": {"crop_meta": torch.zeros(1, 8, device=DEV), "n_crops": torch.zeros(1, dtype=torch.int32, device=DEV),
                    "keypoints": torch.zeros(1, 17, 3, device=DEV)},
           "faces": {"crop_meta": torch.tensor([[0, 0, 2.0, 2.0, 6.0, 4.0, 1.0, 0]], device=DEV),
                     "n_crops": torch.ones(1, dtype=torch.int32, device=DEV), "ident": torch.tensor([-1], device=DEV)}}
    rgb = (200, 40, 90)
    a = Annotator(colour_by="slot", redact="all", redact_mode="fill", redact_rgb=rgb)
    for matrix in ("bt601", "bt709"):
        for rng in ("limited", "full"):
            y, uv, _ = AH.surfaces(1, 10, 12, 1)
            frames = NV12Frames(torch.from_numpy(y).to(DEV), torch.from_numpy(uv).to(DEV), matrix=matrix, range=rng)
            a(frames, out)
            want = AH.A.rgb_to_yuv([rgb], matrix, rng)[0]
            assert frames.y[0, 2:6, 2:8].unique().tolist() == [int(want[0])]
            assert frames.uv[0, 1:3, 1:4].reshape(-1, 2).unique(dim=0).tolist() == [[int(want[1]), int(want[2])]]
            back = frames.to_rgb()[0, 3, 3].tolist()
            assert max(abs(p - q) for p, q in zip(back, rgb)) <= 3
