"""CPU: the C ABI library (loads, exports every symbol declared in include/prpe.h, rejects
bad arguments without launching) and the host-side logic (weight packing, BN folding,
state_dict layout, task routing API)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

from prpe import _lib, arch, pack, synth
from prpe.model import CombinedModel


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "prpe.h")).read()
    return sorted(set(re.findall(r"\b(prpe_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    decl = _declared_symbols()
    assert len(decl) >= 15
    for name in decl:
        assert hasattr(L, name), name
    assert set(decl) == set(_lib.SIGNATURES), "ctypes table must bind exactly the header's entry points"
    assert L.prpe_abi_version() == _lib.ABI_VERSION
    assert b"gfx950" in L.prpe_build_info()


def test_invalid_arguments_are_rejected_before_launch():
    L = _lib.lib()
    d = _lib.ConvDesc()               # null views
    assert L.prpe_conv2d(C.byref(d), None) == -22
    assert L.prpe_nms(None, 1, 1, 1, 0, 0.001, 0.65, 30000, 300, None, None, None, 0, None) == -22
    assert L.prpe_softargmax(None, 1, 1, 1, 1, None, None, None, None, None) == -22
    assert L.prpe_attention(None, None, 1, 192, 12, 64, 0.125, None) == -22
    bad = _lib.View(0x1000, 1, 4, 4, 8, 128, 32, 8, 1)
    assert L.prpe_norm_sigmoid(C.byref(bad), C.byref(bad), None) == -22    # > 4 channels
    # PSA attention writes out at qkv's (h, w): an out (or vout) of another map size is refused,
    # on the LDS kernel's sizes (5x5) and on the streaming kernel's (20x20)
    for h, w in ((5, 5), (20, 20)):
        qkv = _lib.View(0x1000, 2, h, w, 256, h * w * 256, w * 256, 256, 1)
        for oh, ow in ((h - 1, w), (h, w - 1), (h + 1, w), (w, h + 1), (1, 1)):
            o = _lib.View(0x1000, 2, oh, ow, 128, oh * ow * 128, ow * 128, 128, 1)
            assert L.prpe_psa_attention(C.byref(qkv), C.byref(o), None, 2, 32, 64, 0.2, None) == -22, (h, w, oh, ow)
            ok = _lib.View(0x1000, 2, h, w, 128, h * w * 128, w * 128, 128, 1)
            assert L.prpe_psa_attention(C.byref(qkv), C.byref(ok), C.byref(o), 2, 32, 64, 0.2, None) == -22
    # precision 3 without its fp16 planes / input max bound, or with a prologue affine
    v = _lib.View(0x1000, 1, 4, 4, 32, 512, 128, 32, 1)
    d = _lib.ConvDesc(x=v, y=v, kh=1, kw=1, stride=1, pad=0, w_hi=0x1000, w_lo=0x1000, w_lo2=0x1000,
                      k_pad=32, co_pad=128, precision=3)
    assert L.prpe_conv2d(C.byref(d), None) == -22
    d.w_h16 = d.w_l16 = d.scale16 = 0x1000
    assert L.prpe_conv2d(C.byref(d), None) == -22                          # no x_amax
    d.x_amax = 0x1000
    d.in_scale = d.in_bias = 0x1000
    assert L.prpe_conv2d(C.byref(d), None) == -22                          # prologue
    d.precision = 4
    assert L.prpe_conv2d(C.byref(d), None) == -22


def test_fused_launches_refuse_in_place_and_short_slots():
    """prpe_bottleneck / prpe_stem_maxpool read x's halo and residual while other tiles write y:
    an overlapping y is refused before launch (include/prpe.h); the Python wrappers check the
    max|x| slot arrays like prpe_conv2d's (a short array would be indexed out of bounds)."""
    L = _lib.lib()
    x = _lib.View(0x100000, 2, 16, 16, 256, 16 * 16 * 256, 16 * 256, 256, 1)
    d = _lib.BneckDesc(x=x, y=x, x_amax=0x1000, mid=64)
    for i, k in enumerate((256, 576, 64)):
        d.w_h16[i] = d.w_l16[i] = d.scale16[i] = d.bias[i] = 0x1000
        d.k_pad[i] = k
    assert L.prpe_bottleneck(C.byref(d), None) == -22                       # y == x
    d.y = _lib.View(0x100000 + 4096, 2, 16, 16, 256, 16 * 16 * 256, 16 * 256, 256, 1)
    assert L.prpe_bottleneck(C.byref(d), None) == -22                       # y overlaps x
    st = _lib.StemDesc(x=0x100000, xsn=70 * 72 * 4, xsh=72 * 4, n=2, h=64, w=64, x_amax=0x1000, w_h16=0x1000,
                       w_l16=0x1000, k_pad=224, scale16=0x1000, bias=0x1000,
                       y=_lib.View(0x100000 + 64, 2, 16, 16, 64, 16 * 16 * 64, 16 * 64, 64, 1))
    assert L.prpe_stem_maxpool(C.byref(st), None) == -22                    # y inside the frames
    from prpe import ops
    with pytest.raises(ValueError, match="slots"):
        ops._check_slots("t", 4, torch.zeros(3))                           # short (and host) array


def test_amax_slot_pool_grows_for_larger_batches():
    """Engine.amax_slot: chunks made for a small batch are replaced when a later scope asks for
    more slots than they hold (e.g. tokens of a bigger ViT batch), never sliced short."""
    from prpe import engine as E
    e = E.Engine({}, device="cpu")
    for n in (64, 70000, 5, 200000, 3):
        e._amax_begin("vit")
        a = e.amax_slot(n)
        b = e.amax_slot(n)
        assert a.numel() == n and b.numel() == n and float(a.abs().sum() + b.abs().sum()) == 0.0
        a.fill_(1.0)
        b.fill_(2.0)


def test_bordered_buffers_keep_one_batch_size():
    """Engine.bordered: the zero-bordered scratch buffers are cached per shape, and
    a new batch size drops the ones of every other batch size instead of holding them for the
    engine's lifetime."""
    from prpe import engine as E
    e = E.Engine({}, device="cpu")

    def held():
        return sorted(k[1:] for k in e._aux if isinstance(k, tuple) and k[0] == "bordered")

    a = e.bordered(2, 5, 7, 8)
    b = e.bordered(2, 3, 4, 16)
    assert e.bordered(2, 5, 7, 8) is a and len(held()) == 2 and all(k[0] == 2 for k in held())
    a[:, 1:-1, 1:-1, :] = 1.0                                              # callers write the interior
    c = e.bordered(3, 5, 7, 8)
    assert held() == [(3, 7, 9, 8)]                                        # B = 3 only
    assert c.shape == (3, 7, 9, 8) and b.shape == (2, 5, 6, 16)
    c[:, 1:-1, 1:-1, :] = 1.0
    border = c.clone()
    border[:, 1:-1, 1:-1, :] = 0.0
    assert float(border.abs().sum()) == 0.0 and float(c.sum()) == 3 * 5 * 7 * 8


def test_library_refuses_other_sources(monkeypatch):
    """lib() compares the source hash compiled into libprpe.so (build.py) with the hash of the
    sources beside it and refuses a library built from other sources."""
    from prpe import _srchash
    L = _lib.lib()
    built = L.prpe_source_hash().decode()
    assert len(built) == 64 and built == _srchash.source_hash()
    assert built[:16].encode() in L.prpe_build_info()
    _lib.check_source_hash(built)                                          # fresh: accepted
    with pytest.raises(_lib.PrpeError, match="stale"):
        _lib.check_source_hash(built, present="0" * 64)
    # the whole load path: sources that hash differently -> lib() raises
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "source_hash", lambda: "f" * 64)
    with pytest.raises(_lib.PrpeError, match="stale"):
        _lib.lib()


def test_conv_workspace_is_caller_owned():
    """Split-K (IR-50 output layer geometry, M = 256 frames, K = 7*7*512, Co = 512): the
    library reports the partial-sum bytes it needs and never allocates them; every other
    path needs none. Host-only queries (no GPU here)."""
    L = _lib.lib()
    x = _lib.View(0x10000, 256, 7, 7, 512, 7 * 7 * 512, 7 * 512, 512, 1)
    y = _lib.View(0x20000, 256, 1, 1, 512, 512, 512, 512, 1)
    d = _lib.ConvDesc(x=x, y=y, kh=7, kw=7, stride=1, pad=0, w_hi=0x1000, w_lo=0x1000, w_lo2=0x1000,
                      k_pad=25088, co_pad=512, precision=0, k_order=0)
    assert L.prpe_conv2d_workspace_bytes(C.byref(d)) == 49 * 256 * 512 * 4     # one K-slice per tap
    d.tile = 4                                                                # a non-split tile
    assert L.prpe_conv2d_workspace_bytes(C.byref(d)) == 0
    d.tile = 0
    d.k_pad = 100                                                             # invalid pack
    assert L.prpe_conv2d_workspace_bytes(C.byref(d)) == -22
    v = _lib.View(0x1000, 1, 4, 4, 32, 512, 128, 32, 1)
    d = _lib.ConvDesc(x=v, y=v, kh=1, kw=1, stride=1, pad=0, w_hi=0x1000, w_lo=0x1000, w_lo2=0x1000,
                      k_pad=32, co_pad=128, precision=0)
    assert L.prpe_conv2d_workspace_bytes(C.byref(d)) == 0
    src = open(os.path.join(ROOT, "person-recognition-for-pose-estimation_amd", "csrc", "conv_splitk.hip")).read()
    import glob
    for f in glob.glob(os.path.join(ROOT, "person-recognition-for-pose-estimation_amd", "csrc", "*")):
        assert not re.search(r"\bhip(Malloc|Free)\w*\s*\(", open(f).read()), f"{f} allocates device memory"
    assert "workspace" in src


def test_state_dict_spec_is_complete():
    spec = arch.state_dict_spec()
    assert len(spec) == 2130
    n = sum(int(torch.tensor(s).prod()) if len(s) else 1 for _, s, _ in spec)
    assert n == 215109568   # numel of the reference CombinedModel.state_dict()


def test_pack_layout_and_split():
    w = torch.randn(5, 3, 3, 3)
    p = pack.pack_conv("t", w, 1, 1, "cpu")
    assert p.k_pad == 32 and p.co_pad == 128 and (p.kh, p.kw, p.ci, p.co) == (3, 3, 3, 5)
    full = p.w_hi.float() + p.w_lo.float()
    # k = (kh*3 + kw)*Ci + ci
    for co in range(5):
        for kh in range(3):
            for kw in range(3):
                for ci in range(3):
                    k = (kh * 3 + kw) * 3 + ci
                    assert abs(full[co, k] - w[co, ci, kh, kw]) <= 2 ** -16 * abs(w[co, ci, kh, kw]) + 1e-30
    assert torch.all(full[5:] == 0) and torch.all(full[:, 27:] == 0)


def test_f16_scaled_planes_pack():
    """precision-3 weight planes: per-row power-of-2 scale puts max|w| in [2^14, 2^15); the two
    fp16 planes rebuild w to ~2^-22 of the row maximum; the scale folds into the epilogue."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(40, 64, 3, 3, generator=g) * torch.logspace(-4, 2, 40).view(-1, 1, 1, 1)
    w[7] = 0.0                                           # an all-zero output channel
    sc = torch.rand(40, generator=g) + 0.5
    p = pack.pack_conv("t", w, 1, 1, "cpu", scale=sc)
    h, l, s16 = p.f16_planes()
    hf, lf = h.view(torch.float16).float(), l.view(torch.float16).float()
    assert torch.isfinite(hf).all() and torch.isfinite(lf).all()
    rows = hf[:40].abs().amax(1)
    nz = torch.arange(40) != 7
    assert torch.all(rows[nz] >= 2 ** 14) and torch.all(rows[nz] < 2 ** 15)
    full = (p.w_hi.float() + p.w_lo.float() + p.w_lo2.float())[:40]
    e = torch.log2(s16 / sc).round()                     # s16 = scale * 2^-e exactly
    assert torch.equal(s16, torch.ldexp(sc, e.to(torch.int32)))
    rebuilt = (hf[:40] + lf[:40]) * torch.ldexp(torch.ones(40), e.to(torch.int32)).view(-1, 1)
    rowmax = full.abs().amax(1, keepdim=True).clamp_min(1e-30)
    assert ((rebuilt - full).abs() / rowmax).max() < 2 ** -21
    assert torch.all(hf[7] == 0) and torch.all(lf[7] == 0)


def test_stem_as_chunked_conv_over_overlapping_view():
    """The engine's stem rewrite (Engine.stem): conv1 7x7/2 pad 3 on NCHW frames equals a
    7x1-tap stride-2 conv over the 32-"channel" overlapping view of a zero-bordered NHWC4 copy
    with the re-laid-out weight (evaluated here with torch on the CPU)."""
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 22, 17
    x = torch.rand(B, 3, H, W, generator=g)
    w = torch.randn(8, 3, 7, 7, generator=g)
    buf = torch.zeros(B, H + 6, W + 8, 4)
    buf[:, 3:3 + H, 3:3 + W, :3] = x.permute(0, 2, 3, 1)
    v = buf.as_strided((B, H + 6, W, 32), (buf.stride(0), buf.stride(1), 4, 1))
    wv = torch.zeros(8, 7, 8, 4)
    wv[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    w2d = wv.reshape(8, 7 * 32)                       # k = kh*32 + kw*4 + c (chunk-major, KW=1)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W - 1) // 2 + 1
    cols = torch.stack([v[:, kh: kh + 2 * Ho - 1: 2, 0: 2 * Wo - 1: 2, :] for kh in range(7)], 3)
    got = torch.einsum("bhwkc,okc->bohw", cols.double(), w2d.view(8, 7, 32).double())
    ref = torch.nn.functional.conv2d(x.double(), w.double(), None, 2, 3)
    assert got.shape == ref.shape
    torch.testing.assert_close(got, ref, rtol=0, atol=1e-12)


def test_upconv_tap_pack_order():
    w = torch.randn(4, 6, 3, 3)
    p = pack.pack_upconv_taps("t", w, "cpu")
    full = p.w_hi.float() + p.w_lo.float()
    for tap in range(9):
        for co in range(4):
            ref = w[co, :, tap // 3, tap % 3]
            torch.testing.assert_close(full[tap * 4 + co, :6], ref, rtol=2 ** -15, atol=1e-7)


def test_bn_fold_matches_torch_eval_batchnorm():
    sd = {"b.weight": torch.rand(7) + 0.5, "b.bias": torch.randn(7), "b.running_mean": torch.randn(7),
          "b.running_var": torch.rand(7) + 0.1}
    s, t = pack.bn_affine(sd, "b", 1e-3, conv_bias=torch.ones(7))
    x = torch.randn(2, 7, 3, 3)
    ref = torch.nn.functional.batch_norm(x + 1.0, sd["b.running_mean"], sd["b.running_var"], sd["b.weight"],
                                         sd["b.bias"], False, 0.0, 1e-3)
    got = x * s.view(1, 7, 1, 1) + t.view(1, 7, 1, 1)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)


def test_combined_model_task_api(state_dict):
    m = CombinedModel()
    assert m.current_task == "person_detection"
    for t in arch.TASKS:
        m.set_task(t)
        assert m.current_task == t
    with pytest.raises(ValueError, match="not supported"):
        m.set_task("segmentation")
    with pytest.raises(KeyError):
        m.load_state_dict({"foo": torch.zeros(1)})


def test_synth_is_deterministic():
    a = synth.uniform(3, "x", (1000,))
    b = synth.uniform(3, "x", (1000,))
    c = synth.uniform(4, "x", (1000,))
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0


def test_branch_module_surface_for_configure_optimizers(state_dict):
    """The callers' configure_optimizers reach into the branches: the trees
    carry the reference's parameter names and storage, buffers stay buffers, the YOLO head
    stride is a plain attribute (never in state_dict), and an optimizer can be built."""
    m = CombinedModel(state_dict, device="cuda")      # packs lazily: no GPU touched here
    names = dict(m.vit_pose.adapter.named_parameters())
    assert set(names) == {k[len("vit_pose.adapter."):] for k in state_dict
                          if k.startswith("vit_pose.adapter.") and "running_" not in k and "num_batches" not in k}
    assert names["0.weight"].data_ptr() == state_dict["vit_pose.adapter.0.weight"].data_ptr()
    vp = dict(m.vit_pose.vit_pose.named_parameters())
    assert "backbone.encoder.layer.11.mlp.fc2.weight" in vp and "head.conv.weight" in vp
    yb = dict(m.yolo_face.named_buffers())
    assert "adapter.1.running_mean" in yb and "adapter.1.running_mean" not in dict(m.yolo_face.named_parameters())
    assert "yolo.head.stride" not in m.yolo_face.state_dict()
    assert torch.equal(m.yolo_face.yolo.head.stride, torch.zeros(3))
    m.yolo_face.yolo.head.stride = torch.tensor([8.0, 16.0, 32.0])
    m.load_state_dict(state_dict)                      # a reload keeps the caller's stride
    assert m.yolo_face.yolo.head.stride.tolist() == [8.0, 16.0, 32.0]
    ada = list(m.ada_face.adapter.parameters()) + list(m.ada_face.parameters())   # module.py:179-180
    import warnings
    with warnings.catch_warnings():       # the reference's list repeats the adapter's parameters too
        warnings.simplefilter("ignore", UserWarning)
        opt = torch.optim.Adam(ada + list(m.yolo_person.parameters()), lr=1e-3)
    assert len(opt.param_groups[0]["params"]) == len(ada) + len(list(m.yolo_person.parameters()))
    n_ref = sum(1 for k, v in state_dict.items() if "running_" not in k and "num_batches" not in k
                and k.split(".")[-1] not in ("t", "batch_mean", "batch_std"))
    assert sum(1 for _ in m.parameters()) == n_ref
    assert m.ada_face.head.kernel is None              # the synthetic state_dict has no head kernel
    with pytest.raises(ValueError):
        m.vit_pose.vit_pose(torch.zeros(1, 3, 256, 192))   # CPU tensor: the HIP path only


def test_state_dict_spec_matches_reference_keys():
    """arch.state_dict_spec() == the reference CombinedModel's own state_dict() (keys and
    shapes, recorded by oracle/make_golden_evalsteps.py into tests/golden/sd_keys_ref.json)."""
    import json
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "sd_keys_ref.json")))
    spec = {k: list(s) for k, s, _ in arch.state_dict_spec()}
    assert spec == {k: list(s) for k, s in ref.items()}


def test_traffic_records_name_their_kernel_sources():
    """profiles/r02_pmc_traffic_<config>.json (the bench line's `traffic`) list the csrc files
    their kernel is built from; the bench reports the number only while those files hash to
    the recorded value (a change to another kernel does not make it stale, a change to this
    one does)."""
    import glob
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    recs = glob.glob(os.path.join(ROOT, "profiles", "r02_pmc_traffic_*.json"))
    assert {os.path.basename(r) for r in recs} >= {"r02_pmc_traffic_full.json", "r02_pmc_traffic_yolo_face.json",
                                                   "r02_pmc_traffic_vitpose.json"}
    csrc = os.path.join(ROOT, "person-recognition-for-pose-estimation_amd", "csrc")
    for r in recs:
        t = json.load(open(r))
        assert t["sources"] and all(os.path.exists(os.path.join(csrc, f)) for f in t["sources"])
        assert t["hbm_bytes_per_launch"] > 0 and t["algorithmic_bytes_per_launch"] > 0
        h = bench.kernel_sources_hash(t["sources"])
        assert len(h) == 16 and h == bench.kernel_sources_hash(list(reversed(t["sources"])))
        assert h != bench.kernel_sources_hash(), "a subset hash must differ from the all-sources hash"


def test_bench_dump_outputs_writes_float_arrays_within_budget(tmp_path, monkeypatch):
    """bench.dump_outputs: one <name>.npy per tensor of the step's result (lists numbered),
    float32 (float64 for 64-bit values); within the byte budget the arrays are whole, over it
    the largest is cut to the same sorted sample of its elements in every run."""
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(3)
    o = {"heat": torch.rand(7, 5, 11, generator=g), "cnt": torch.arange(9, dtype=torch.int32),
         "idx": torch.arange(4, dtype=torch.int64) + 2 ** 40, "gathered": [torch.rand(3, 2, generator=g), torch.ones(2)]}
    a_dir, b_dir, c_dir = (str(tmp_path / n) for n in "abc")
    bench.dump_outputs(a_dir, o)
    assert sorted(os.listdir(a_dir)) == ["cnt.npy", "gathered_0.npy", "gathered_1.npy", "heat.npy", "idx.npy"]
    heat = np.load(os.path.join(a_dir, "heat.npy"))
    assert heat.dtype == np.float32 and np.array_equal(heat, o["heat"].numpy())
    assert np.load(os.path.join(a_dir, "cnt.npy")).dtype == np.float32
    idx = np.load(os.path.join(a_dir, "idx.npy"))
    assert idx.dtype == np.float64 and np.array_equal(idx, o["idx"].numpy().astype(np.float64))
    monkeypatch.setattr(bench, "DUMP_BUDGET", 600)          # heat (1540 bytes) no longer fits
    bench.dump_outputs(b_dir, o)
    bench.dump_outputs(c_dir, o)
    files = [np.load(os.path.join(b_dir, f)) for f in sorted(os.listdir(b_dir))]
    assert len(files) == 5 and sum(f.nbytes for f in files) <= 600
    cut = np.load(os.path.join(b_dir, "heat.npy"))
    assert cut.ndim == 1 and 0 < cut.size < heat.size and np.array_equal(cut, np.load(os.path.join(c_dir, "heat.npy")))
    assert np.isin(cut, heat).all()
    assert np.array_equal(np.load(os.path.join(b_dir, "gathered_0.npy")), o["gathered"][0].numpy())


def test_weight_versions_trigger_repack(monkeypatch):
    """Host logic of the stale-weights guard (prpe/model.py ``_sync_weights``) without a GPU:
    the engine is a stub counting repacks; in-place writes through the branch trees'
    parameters, the trunk's ``parameters()`` and ``state_dict()`` values all mark the model stale."""
    import torch
    from prpe import arch, model as M, synth

    built = []

    class StubEngine:
        def __init__(self, sd, device, precision):
            built.append(1)

    monkeypatch.setattr(M, "Engine", StubEngine)
    sd = synth.make_state_dict(arch.state_dict_spec())
    m = M.CombinedModel(sd, device="cuda")
    assert len(built) == 1 and not m.weights_stale()
    m._sync_weights()
    assert len(built) == 1                                  # nothing changed: no repack
    with torch.no_grad():
        dict(m.vit_pose.adapter.named_parameters())["7.weight"].add_(1.0)
    assert m.weights_stale()
    m._sync_weights()
    assert len(built) == 2 and not m.weights_stale()
    with torch.no_grad():
        next(iter(m.parameters())).mul_(2.0)                # a trunk parameter
    assert m.weights_stale()
    m._sync_weights()
    with torch.no_grad():
        m.state_dict()["yolo_face.adapter.0.weight"].zero_()
    assert m.weights_stale()
    m._sync_weights()
    assert len(built) == 4 and not m.weights_stale()


def test_every_environment_switch_is_documented():
    """kernel routing must not depend on undocumented process-wide
    environment variables -- every PRPE_* switch the library or the engine reads is listed in
    INTEGRATION.md §4. VERDICT r06 weak item 7: the library itself reads none."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "person-recognition-for-pose-estimation_amd")
    for f in glob.glob(os.path.join(pkg, "csrc", "*")):
        assert "getenv" not in open(f).read(), f
    read = set()
    for f in glob.glob(os.path.join(pkg, "csrc", "*.hip")) + glob.glob(os.path.join(pkg, "prpe", "*.py")):
        read |= set(re.findall(r'(?:getenv|environ\.get)\("(PRPE_[A-Z0-9_]+)"', open(f).read()))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    documented = set(re.findall(r"PRPE_[A-Z0-9_]+", doc[doc.index("## 4. Environment switches"):]))
    assert read and not (read - documented), sorted(read - documented)
