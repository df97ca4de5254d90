"""GPU: prpe_frame_ingest_multi (csrc/ingest_multi.hip) -- mixed-size uint8 frames
with an antialiased downscale, held BIT FOR BIT to the numpy fp32 restatement of
tests/test_ingest_multi_host.py (``ingest_multi_ref``, which that file pins to torch's own
antialias), to prpe_frame_ingest frame by frame with filter 0, and to itself across batch sizes,
positions, chunks and runs. Every case writes into the interior of a sentinel-filled, bordered
buffer and checks that nothing else moved. No tolerance appears in this file: every comparison is
of bits.

"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_ingest_multi_host as M
from prpe import CombinedModel, FrameIngest, _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.0                                     # no case writes this value
FILL = (114.0, 0.0, 255.0)
LAYOUTS = ("hwc", "nchw_permuted", "slice")


def to_dev(frame, layout="hwc"):
    """A source frame on the device as [Hs, Ws, 3] with the strides of an HWC image, of an NCHW
    tensor seen through ``permute``, or of a window of a wider image."""
    t = torch.from_numpy(np.ascontiguousarray(frame))
    Hs, Ws, _ = t.shape
    if layout == "nchw_permuted":
        d = t.permute(2, 0, 1).contiguous().to(DEV).permute(1, 2, 0)
        assert d.stride(2) == Hs * Ws
        return d
    if layout == "slice":
        wide = torch.full((Hs + 3, Ws + 5, 3), 77, dtype=torch.uint8)
        wide[2:2 + Hs, 4:4 + Ws] = t
        d = wide.to(DEV)[2:2 + Hs, 4:4 + Ws]
        assert d.stride(0) == (Ws + 5) * 3
        return d
    return t.to(DEV)


def run(frames, size, geoms, filt, a, b, fill=FILL, swap=False, around=(0, 0)):
    """The op into the interior of frames [lead, lead + B) of a sentinel-filled stem-shaped buffer
    [lead + B + trail, H + 6, W + 8, 4]; returns (the B interiors [B, H, W, 4], y_amax [B]) on the
    host after asserting that the border and the other frames still hold the sentinel."""
    H, W = size
    lead, trail = around
    B = len(frames)
    buf = torch.full((lead + B + trail, H + 6, W + 8, 4), SENT, device=DEV)
    amax = torch.zeros(B, device=DEV)
    y = buf[lead:lead + B, 3:3 + H, 3:3 + W, :]
    assert ops.frame_ingest_multi(frames, y, geoms, filt, a, b, fill, swap, y_amax=amax) is y
    out = buf.cpu()
    touched = torch.zeros_like(out, dtype=torch.bool)
    touched[lead:lead + B, 3:3 + H, 3:3 + W, :] = True
    assert bool((out[~touched] == SENT).all()), "the border or another frame was written"
    return out[lead:lead + B, 3:3 + H, 3:3 + W, :].contiguous(), amax.cpu()


def bits(t):
    t = torch.from_numpy(np.array(t)) if isinstance(t, np.ndarray) else t
    return t.contiguous().view(torch.int32)


def same(got, want):
    return tuple(got.shape) == tuple(want.shape) and torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------ filter 1 against the restatement
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_antialias_case_is_bit_equal_to_the_restatement(name):
    frame, size, geom, a, b, fill, swap = M.case(name)
    layout = LAYOUTS[sorted(M.CASES).index(name) % 3]
    got, amax = run([to_dev(frame, layout)], size, [geom], 1, a, b, fill, swap, around=(1, 1))
    want = M.ref_of(name)
    assert same(got[0], want), name
    assert float(amax[0]) == float(np.abs(want).max())                # the whole interior, fill included


MIXED = (((64, 96), "stretch"), ((97, 131), "letterbox"), ((1024, 33), "stretch"), ((7, 480), "letterbox"),
         ((33, 20), "stretch"))                                        # the last one is magnified on x


@pytest.fixture(scope="module")
def mixed():
    """Five sizes into 32 x 48, one norm and channel order: frames, regions, restatements (shared)."""
    a, b = M.norm_ab("imagenet")
    frames = [M.frame_of(Hs, Ws, 40 + n) for n, ((Hs, Ws), _) in enumerate(MIXED)]
    geoms = [FrameIngest(size=(32, 48), mode=mode).geometry(*hw) for hw, mode in MIXED]
    refs = [M.ingest_multi_ref(f, g, a, b, FILL, True, True, (32, 48)) for f, g in zip(frames, geoms)]
    for r in refs:
        r.setflags(write=False)
    return frames, geoms, a, b, refs


def test_mixed_batch_of_five_sizes(mixed):
    frames, geoms, a, b, refs = mixed
    dev = [to_dev(f, LAYOUTS[n % 3]) for n, f in enumerate(frames)]
    got, amax = run(dev, (32, 48), geoms, 1, a, b, FILL, True, around=(1, 0))
    for n, want in enumerate(refs):
        assert same(got[n], want), MIXED[n]
        assert float(amax[n]) == float(np.abs(want).max())
    again, amax2 = run(dev, (32, 48), geoms, 1, a, b, FILL, True, around=(1, 0))
    assert same(again, got) and same(amax2, amax)                     # two runs, the same bytes


def test_batch_independence_across_positions_chunks_and_order(mixed):
    """The frame alone, at index 0, at index 31 and at index 32 (the second launch: chunks hold 32
    frames) of a 33-frame batch, and the batch reversed: the same bytes every time."""
    frames, geoms, a, b, refs = mixed
    dev = [to_dev(f) for f in frames]
    order = [1 if n in (0, 31, 32) else (0, 2, 3, 4)[n % 4] for n in range(33)]
    got, amax = run([dev[k] for k in order], (32, 48), [geoms[k] for k in order], 1, a, b, FILL, True)
    alone, amax1 = run([dev[1]], (32, 48), [geoms[1]], 1, a, b, FILL, True)
    assert same(alone[0], refs[1])
    for n, k in enumerate(order):
        assert same(got[n], refs[k]), (n, k)
        assert float(amax[n]) == float(np.abs(refs[k]).max())
    for n in (0, 31, 32):
        assert same(got[n], alone[0]) and float(amax[n]) == float(amax1[0])
    rev = order[::-1]
    got_r, amax_r = run([dev[k] for k in rev], (32, 48), [geoms[k] for k in rev], 1, a, b, FILL, True)
    assert same(got_r, got.flip(0)) and same(amax_r, amax.flip(0))


# ------------------------------------------------------------------ filter 0 is prpe_frame_ingest
@pytest.mark.parametrize("swap,norm", [(False, "unit"), (True, "imagenet")])
def test_bilinear_is_frame_ingest_frame_by_frame(mixed, swap, norm):
    frames, geoms, _, _, _ = mixed
    a, b = M.norm_ab(norm)
    dev = [to_dev(f, LAYOUTS[(n + 1) % 3]) for n, f in enumerate(frames)]
    got, amax = run(dev, (32, 48), geoms, 0, a, b, FILL, swap, around=(0, 1))
    for n, (f, g) in enumerate(zip(dev, geoms)):
        buf = torch.full((1, 38, 56, 4), SENT, device=DEV)
        one = torch.zeros(1, device=DEV)
        ops.frame_ingest(f[None], buf[:, 3:35, 3:51, :], g, a, b, FILL, swap, y_amax=one)
        assert same(got[n], buf[0, 3:35, 3:51, :].cpu()), MIXED[n]
        assert float(amax[n]) == float(one[0])
    # and the restatement with antialias off says the same (what the host file pins to torch)
    want = M.ingest_multi_ref(frames[1], geoms[1], a, b, FILL, swap, False, (32, 48))
    assert same(got[1], want)


@pytest.mark.parametrize("filt", [0, 1])
def test_equal_size_has_the_bits_of_float_times_a_plus_b(filt):
    a, b = (0.0123, -0.5, 1 / 255), (-1.5, 3.25, 0.1)
    frames = [M.frame_of(32, 48, 60), M.frame_of(32, 48, 61) // 4]
    got, amax = run([to_dev(frames[0], "nchw_permuted"), to_dev(frames[1], "slice")], (32, 48), [(0, 0, 32, 48)] * 2,
                    filt, a, b, FILL, True)
    for n, f in enumerate(frames):
        want = torch.from_numpy(f.copy()).flip(2).float() * torch.tensor(a) + torch.tensor(b)
        assert same(got[n, :, :, :3], want) and not bool(got[n, :, :, 3].any())
        assert float(amax[n]) == float(want.abs().max())
    assert float(amax[0]) != float(amax[1])


def test_y_amax_is_the_maximum_over_the_interior_fill_included():
    """A letterboxed dark frame whose fill dominates, and a bright one whose pixels do."""
    a, b = M.norm_ab("unit")
    dark, bright = M.frame_of(270, 480, 70) // 8, 240 + M.frame_of(270, 480, 71) % 16
    geom = FrameIngest(size=(64, 64)).geometry(270, 480)
    got, amax = run([to_dev(dark), to_dev(bright)], (64, 64), [geom] * 2, 1, a, b, (200.0, 200.0, 200.0))
    for n in range(2):
        assert float(amax[n]) == float(got[n].abs().max())
    fv = float(np.float32(200.0) * np.float32(a[0]) + np.float32(b[0]))
    assert float(amax[0]) == abs(fv) and float(amax[1]) > float(amax[0])


@pytest.mark.parametrize("src", [(64, 96), (97, 131), (1024, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("value", [0, 255])
def test_constant_frames(value, src):
    """An all-zero and an all-255 frame give exactly b and 255 * a + b, at integer and non-integer
    scales: the sums are over differences from the first tap, so the weights cannot drift them."""
    a, b = M.norm_ab("imagenet")
    frame = np.full(src + (3,), value, np.uint8)
    got, _ = run([to_dev(frame)], (32, 48), [(0, 0, 32, 48)], 1, a, b)
    want = np.float32(value) * np.asarray(a, np.float32) + np.asarray(b, np.float32)
    dev = np.abs(got[0, :, :, :3].numpy().astype(np.float64) - want.astype(np.float64)).max()
    print(f"constant {value} from {src}: max |y - ({value} * a + b)| = {dev:.3e}")
    assert same(got[0, :, :, :3], np.ascontiguousarray(np.broadcast_to(want, (32, 48, 3))))


# ------------------------------------------------------------------ through the public interface
@pytest.fixture(scope="module")
def model(state_dict):
    return CombinedModel(state_dict, device=DEV)


def _tensors(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _tensors(o)]
    return [out.heatmaps]


def test_forward_u8_on_a_list_of_three_sizes_equals_each_frame_alone(model):
    ing = FrameIngest(size=(64, 64), norm="imagenet", channel_order="bgr", antialias=True)
    frames = [to_dev(M.frame_of(97, 131, 80), "slice"), to_dev(M.frame_of(64, 64, 81)),
              to_dev(M.frame_of(270, 480, 82), "nchw_permuted")]
    got = _tensors(model.forward_u8(frames, ing))
    assert got and all(t.shape[0] == 3 for t in got)
    for n, f in enumerate(frames):
        for g, w in zip(got, _tensors(model.forward_u8([f], ing))):
            assert same(g[n:n + 1].cpu(), w.cpu()), n
    all_heads = model.forward_all_u8(frames, ing, face_stride=[8.0, 16.0, 32.0])
    assert all_heads["heatmaps"].shape[0] == 3 and float(all_heads["heatmaps"].abs().max()) > 0.0
    with pytest.raises(ValueError, match="whole-frame ingest only"):
        from prpe import TopDownPose
        TopDownPose(model).from_frames_u8(frames, ing)


def test_four_d_tensor_without_antialias_takes_todays_launch(model, monkeypatch):
    g = torch.Generator().manual_seed(24)
    u8 = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8)
    ing = FrameIngest(size=(64, 64), mode="stretch", norm="unit")
    x = (u8.permute(0, 3, 1, 2).float() * torch.tensor(ing.a).view(1, 3, 1, 1)
         + torch.tensor(ing.b).view(1, 3, 1, 1)).to(DEV)
    want = _tensors(model(x))
    via_multi = _tensors(model.forward_u8(u8.to(DEV), FrameIngest(size=(64, 64), mode="stretch", norm="unit",
                                                                  antialias=True)))

    def never(*args, **kw):
        raise AssertionError("a 4-D tensor with antialias=False went through prpe_frame_ingest_multi")

    monkeypatch.setattr(ops, "frame_ingest_multi", never)
    today = _tensors(model.forward_u8(u8.to(DEV), ing))
    for t, v, w in zip(today, via_multi, want):
        assert same(t.cpu(), w.cpu()) and same(v.cpu(), w.cpu())       # equal size: the same bits either way


def test_to_source_with_sizes_maps_a_box_per_frame():
    ing = FrameIngest(size=(640, 640))
    sizes = [(720, 1280), (2160, 3840), (1920, 1080)]
    g = torch.Generator().manual_seed(6)
    boxes = (torch.rand(3, 5, 4, generator=g) * 640).to(DEV)
    src = ing.to_source(boxes, sizes)
    assert src.device == boxes.device and src.shape == boxes.shape
    for n, (Hs, Ws) in enumerate(sizes):
        one = ing.to_source(boxes[n], Hs, Ws)
        assert float((src[n] - one).abs().max()) <= 4 * max(Hs, Ws) * 2.0 ** -24
        top, left, nh, nw = ing.geometry(Hs, Ws)
        corner = torch.tensor([[left, top, left + nw, top + nh]], dtype=torch.float32, device=DEV)
        want = torch.tensor([[0.0, 0.0, Ws, Hs]], device=DEV)
        full = ing.to_source(corner.expand(3, 1, 4), sizes)[n]
        assert float((full - want).abs().max()) <= 1e-3
    assert float((ing.to_model(src, sizes) - boxes).abs().max()) <= 8 * 640 * 2.0 ** -24


# ------------------------------------------------------------------ refusals launch nothing
def test_refusals_leave_the_buffer_alone():
    a, b = M.norm_ab("unit")
    f = to_dev(M.frame_of(97, 131, 90))
    cpu = torch.from_numpy(M.frame_of(8, 8, 91))
    buf = torch.full((2, 38, 56, 4), SENT, device=DEV)
    y = buf[:, 3:35, 3:51, :]
    ok = (0, 0, 32, 48)
    over = to_dev(np.zeros((1025, 33, 3), np.uint8))                  # the first size above scale 32
    for frames, geoms, filt, dst in (([f, f], [ok, (0, 0, 33, 48)], 1, y), ([f, f], [ok, (1, 1, 32, 48)], 0, y),
                                     ([f, f], [(0, 0, 0, 48), ok], 1, y), ([f, over], [ok, ok], 1, y),
                                     ([f, cpu], [ok, ok], 1, y), ([f], [ok], 1, y), ([f, f, f], [ok] * 3, 0, y),
                                     ([f, f], [ok, ok], 2, y), ([f, f], [ok, ok], 1, buf[:, 3:35, 3:51, :3]),
                                     ([f, f.float()], [ok, ok], 0, y)):
        with pytest.raises(ValueError):
            ops.frame_ingest_multi(frames, dst, geoms, filt, a, b)
    # 1024 x 33 is scale 32 exactly and is taken (test_antialias_case...[scale_32]); the library itself:
    L, f3 = _lib.lib(), (C.c_float * 3)(1.0, 1.0, 1.0)
    row = lambda t, g: _lib.IngestSrc(t.data_ptr(), t.shape[0], t.shape[1], *t.stride(), *g)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rows, filt in (([row(f, ok), row(over, ok)], 1), ([row(f, ok), row(f, (0, 0, 32, 49))], 0),
                       ([row(f, ok), row(f, ok)], 2), ([row(f, ok), _lib.IngestSrc(None, 8, 8, 24, 3, 1, *ok)], 1)):
        t = (_lib.IngestSrc * 2)(*rows)
        assert L.prpe_frame_ingest_multi(t, 2, C.byref(ops.view(y)), filt, f3, f3, f3, 0, None, stream) == -22
    assert L.prpe_frame_ingest_multi((_lib.IngestSrc * 2)(row(f, ok), row(f, ok)), 2, C.byref(ops.view(buf[:1, 3:35, 3:51])),
                                     1, f3, f3, f3, 0, None, stream) == -22              # B != y->n
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
