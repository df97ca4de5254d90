"""GPU: the launch plan of prpe.engine -- which library call every forward makes, in order, with
the arguments the engine decides -- against goldens under tests/golden/launch_plan/.

The kernel suites pin the C ABI; this pins the Python routing above it: the precision each conv
takes (and every fallback of Engine._f16_ok / _bneck_ok / feat_prec), the planes-format handoffs,
the fused launches, and the producer -> consumer wiring of the per-frame max|x| slots.

Every public function of prpe.ops is wrapped (monkeypatch on the module attribute; the wrapped
function still runs) and writes one line per call:

* conv2d: pack name, p<precision>, the views x y res x2 y2 (shape, and /s<strides> unless they are
  the row-major strides of that shape), then t=<tile> act= rm=<res_mode> xp= yp= (planes flags)
  w2= w3= (present or not) act2=, each only where it is not the default (0, the pack's act, 0, 0,
  0, 0, 0, none), then the slots.
* slots (x_amax / y_amax / x2_amax of conv2d, bottleneck, stem_maxpool, upconv3x3, copy_pad,
  frame_ingest): ``slot<k>``, k numbering the distinct (data_ptr, numel) pairs in order of first
  appearance within the recorded forward. A consumer's x_amax must be its producer's y_amax.
* every other op: its name and every argument by parameter name: tensors as dtype, shape and
  strides, packs by name, scalars and flags by value.
* an argument that is None is left out of its line. No device address and no value computed on
  the device is recorded.

Random weights, Engine.prepare() done first, frames 2 x 3 x 64 x 96 (the smallest size with
H % 4 == 0, W % 4 == 0 and H != W, so the fused stem + pool runs; the adapters upsample to fixed
sizes, so the heads run their real shapes).

The goldens are gzipped text, one file per forward (14 forwards are 270 KB of very repetitive
lines): ``zcat tests/golden/launch_plan/a_forward_all.txt.gz`` shows one.

Regenerating: PRPE_LAUNCH_PLAN_REGEN=1 in the environment rewrites the goldens from this run
instead of comparing. Do that only in a change that means to alter the plan, and say in it which
lines changed and why.
"""
import gzip
import inspect
import os

import pytest
import torch

from prpe import CombinedModel, TopDownPose, ops
from prpe import engine as E
from prpe.pack import ConvPack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan")
REGEN = os.environ.get("PRPE_LAUNCH_PLAN_REGEN", "0") == "1"
STRIDE = [8.0, 16.0, 32.0]
SWITCHES = ("PLANES_ON", "SMALLCO_TAPS", "TAPS_FUSE", "BNECK_FUSE", "BNECK_PROJ", "BNECK_L2", "STEM_POOL",
            "PATCH_VIEW", "T1_BORDER")
NOT_LAUNCHES = ("view", "nhwc", "gallery_plan")         # host-only helpers of prpe.ops
SLOTS = ("x_amax", "y_amax", "x2_amax")
_DT = {torch.float32: "f32", torch.uint8: "u8", torch.int32: "i32", torch.int64: "i64", torch.float64: "f64"}


def _tensor(t, dtype=True):
    s = (_DT.get(t.dtype, str(t.dtype)) if dtype else "") + "[" + ",".join(str(v) for v in t.shape) + "]"
    dense, acc = [], 1
    for n in reversed(t.shape):
        dense.insert(0, acc)
        acc *= n
    if tuple(t.stride()) != tuple(dense):
        s += "/s" + ",".join(str(v) for v in t.stride())
    return s


def _value(v):
    if isinstance(v, torch.Tensor):
        return _tensor(v)
    if isinstance(v, ConvPack):
        return v.name
    if isinstance(v, bool):
        return str(int(v))
    if isinstance(v, (int, float, str)):
        return repr(v) if isinstance(v, float) else str(v)
    if isinstance(v, (list, tuple)):
        return "(" + ",".join(_value(x) for x in v) + ")"
    return type(v).__name__


class Recorder:
    def __init__(self, monkeypatch):
        self.lines, self.slots = None, {}
        for name, fn in list(vars(ops).items()):
            if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not name.startswith("_") and \
                    name not in NOT_LAUNCHES:
                monkeypatch.setattr(ops, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def call(*args, **kw):
            if self.lines is not None:
                b = sig.bind(*args, **kw)
                b.apply_defaults()
                self.lines.append((self._conv2d if name == "conv2d" else self._generic)(name, b.arguments))
            return fn(*args, **kw)
        return call

    def _slot(self, t):
        key = (t.data_ptr(), t.numel())
        return "slot%d" % self.slots.setdefault(key, len(self.slots))

    def _generic(self, name, a):
        out = [name]
        for k, v in a.items():
            if v is not None:
                out.append(f"{k}={self._slot(v) if k in SLOTS else _value(v)}")
        return " ".join(out)

    def _conv2d(self, name, a):
        out = [name, a["pack"].name, f"p{a['precision']}"]
        out += [f"{k}={_tensor(a[k], dtype=False)}" for k in ("x", "y", "res", "x2", "y2") if a[k] is not None]
        flags = (("t", a["tile"], 0), ("act", a["act"], None), ("rm", a["res_mode"], 0), ("xp", int(a["x_planes"]), 0),
                 ("yp", int(a["y_planes"]), 0), ("w2", int(a["w2"] is not None), 0), ("w3", int(a["w3"] is not None), 0),
                 ("act2", a["act2"], "none"))
        out += [f"{k}={v}" for k, v, default in flags if v != default]
        out += [f"{k}={self._slot(a[k])}" for k in SLOTS if a[k] is not None]
        return " ".join(out)

    def record(self, forward):
        self.lines, self.slots = [], {}
        try:
            forward()
            torch.cuda.synchronize()
            return self.lines
        finally:
            self.lines = None


@pytest.fixture(autouse=True)
def _default_environment():
    """A changed switch or environment routes launches differently: fail, never compare another plan."""
    changed = [s for s in SWITCHES if getattr(E, s) is not True]
    assert not changed, f"prpe.engine switches not at their defaults: {changed}"
    for var in ("PRPE_ADAFACE_PREC", "PRPE_IR50_OUT_TILE"):
        assert var not in os.environ, f"{var} is set: the launch plan is pinned for the default environment"


@pytest.fixture(scope="module")
def model_of(state_dict):
    """CombinedModel per precision policy, packs built (Engine.prepare), shared by the cases."""
    models = {}

    def get(precision):
        key = repr(precision)
        if key not in models:
            models[key] = CombinedModel(state_dict, device=DEV, precision=precision)
            models[key].engine.prepare()
        return models[key]
    return get


def _frames():
    return torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(11)).to(DEV)


def _frames_u8():
    return torch.randint(0, 256, (2, 48, 80, 3), generator=torch.Generator().manual_seed(12), dtype=torch.uint8).to(DEV)


def _task(m, task):
    m.set_task(task)
    return m(_frames())


def _stale_trunk(m):
    e = m.engine
    f1 = e.trunk(_frames())
    e.trunk(_frames())                     # re-zeroes the trunk pool: f1's slots are stale (feat_prec)
    return e.yolo("yolo_face", f1, STRIDE)


def _flip_pose(m):
    e = m.engine
    return e.vitpose(e.trunk(_frames(), flip_w=True))


# case -> (precision policy, forward(model))
CASES = {
    "a_forward_all": ("auto", lambda m: m.forward_all(_frames(), face_stride=STRIDE, concurrent=False)),
    "b_forward_all_u8": ("auto", lambda m: m.forward_all_u8(_frames_u8(), face_stride=STRIDE, concurrent=False)),
    "c_face_detection": ("auto", lambda m: _task(m, "face_detection")),
    "c_person_detection": ("auto", lambda m: _task(m, "person_detection")),
    "c_pose_estimation": ("auto", lambda m: _task(m, "pose_estimation")),
    "c_face_recognition": ("auto", lambda m: _task(m, "face_recognition")),
    "c_pose_from_pixel_values": ("auto", lambda m: m.vitpose_from_pixels(
        torch.rand(2, 3, 256, 192, generator=torch.Generator().manual_seed(13)).to(DEV))),
    "d_yolo_raw": ("auto", lambda m: m.engine.yolo_raw("yolo_face", _frames(), STRIDE)),
    "e_topdown_3_crops": ("auto", lambda m: TopDownPose(m, max_crops=3)(_frames())),
    "f_flip_trunk_vitpose": ("auto", _flip_pose),
    "g_forward_all_prec2": (2, lambda m: m.forward_all(_frames(), face_stride=STRIDE, concurrent=False)),
    "h_forward_all_prec0": (0, lambda m: m.forward_all(_frames(), face_stride=STRIDE, concurrent=False)),
    "i_forward_all_adaface3": ({"adaface": 3},
                               lambda m: m.forward_all(_frames(), face_stride=STRIDE, concurrent=False)),
    "j_head_on_stale_trunk": ("auto", _stale_trunk),
}


@pytest.mark.parametrize("case", list(CASES))
def test_launch_plan_matches_golden(case, model_of, monkeypatch):
    precision, forward = CASES[case]
    m = model_of(precision)
    task = m.current_task
    rec = Recorder(monkeypatch)
    try:
        plan = rec.record(lambda: forward(m))
    finally:
        m.set_task(task)
    assert plan, "no library call recorded"
    path = os.path.join(GOLDEN, case + ".txt.gz")
    if REGEN:
        os.makedirs(GOLDEN, exist_ok=True)
        with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
            f.write(("\n".join(plan) + "\n").encode())
    with gzip.open(path, "rt") as f:
        want = f.read().splitlines()
    for i, (got, exp) in enumerate(zip(plan, want)):
        if got != exp:
            print(f"{case}: first difference at line {i}\n  recorded: {got}\n  golden:   {exp}")
            pytest.fail(f"{case}: launch plan differs from the golden at line {i}: {got!r} != {exp!r}")
    n = min(len(plan), len(want))
    assert len(plan) == len(want), (f"{case}: {len(plan)} calls recorded, {len(want)} in the golden; line {n} is only "
                                    f"in the {'recording' if len(plan) > n else 'golden'}: {(plan + want[n:])[n]!r}")
