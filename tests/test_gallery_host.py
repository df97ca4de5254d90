"""CPU (no GPU): the face-identification stage's host side.

* the ABI table: the three gallery entry points, declared, bound and exported, at ABI 12;
* every bad argument is refused with -22 before any launch (the pointers below are never read);
* ``gallery_topk_ref``, the plain-torch restatement of the search's semantics (include/prpe.h) that
  the GPU tests use in fp64 as their yardstick, on hand-made cases;
* ``ops.gallery_plan`` against the library's own workspace size (both restate one launch plan);
* ``FaceGallery`` bookkeeping with the ``ops`` calls stubbed.
"""
import os
import re

import pytest
import torch

from conftest import ROOT
from prpe import _lib

EPS = 1e-12


def gallery_topk_ref(queries, gallery, k, valid=None, labels=None, threshold=None, dtype=torch.float64):
    """(scores [Q, k], rows [Q, k] int32[, ident [Q] int64]) by the stated rule: both sides
    normalised as F.normalize does (x / max(||x||, 1e-12)), score = their dot product in ``dtype``,
    rows with a zero valid byte and scores that are not finite skipped, order (-score, row) by a
    stable sort, (-inf, -1) past the number of candidates."""
    def normalise(x):
        x = x.to(dtype)
        return x / x.norm(dim=1, keepdim=True).clamp_min(EPS)

    s = normalise(queries) @ normalise(gallery).t()
    skip = ~torch.isfinite(s)
    if valid is not None:
        skip |= (valid.reshape(1, -1) == 0)
    s = torch.where(skip, torch.full_like(s, float("-inf")), s)
    if s.shape[1] < k:
        s = torch.cat([s, torch.full((s.shape[0], k - s.shape[1]), float("-inf"), dtype=dtype)], 1)
    top, rows = torch.sort(s, dim=1, descending=True, stable=True)
    top, rows = top[:, :k], rows[:, :k].to(torch.int32)
    rows = torch.where(torch.isinf(top), torch.full_like(rows, -1), rows)
    if labels is None:
        return top, rows
    hit = (rows[:, 0] >= 0) & (top[:, 0] >= threshold)
    ident = torch.where(hit, labels[rows[:, 0].clamp(min=0).long()], torch.full((s.shape[0],), -1, dtype=torch.int64))
    return top, rows, ident


# ---------------------------------------------------------------------------------- ABI
NAMES = (("int", "prpe_gallery_enrol", 9), ("int64_t", "prpe_gallery_topk_workspace_bytes", 3),
         ("int", "prpe_gallery_topk", 16))


def test_abi_table_has_the_gallery_entry_points():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert _lib.ABI_VERSION == 12
    assert int(re.search(r"#define PRPE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for res, name, nargs in NAMES:
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\b" + res + " " + name + r"\s*\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/prpe.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().prpe_abi_version() == 12


def _enrol(L, x=0x1000, ld=512, n=4, D=512, gal=0x2000, norms=0x3000, cap=16, row0=0):
    return L.prpe_gallery_enrol(x, ld, n, D, gal, norms, cap, row0, None)


def _topk(L, q=0x1000, ld=512, Q=2, D=512, gal=0x2000, G=100, valid=None, k=5, scores=0x3000, rows=0x4000,
          labels=None, thr=0.0, ident=None, ws=0x10000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.prpe_gallery_topk_workspace_bytes(Q, G, min(max(k, 1), 8))
    return L.prpe_gallery_topk(q, ld, Q, D, gal, G, valid, k, scores, rows, labels, thr, ident, ws, ws_bytes, None)


def test_library_rejects_bad_gallery_arguments_before_launch():
    L = _lib.lib()
    for kw in (dict(x=None), dict(gal=None), dict(norms=None), dict(n=0), dict(D=48), dict(D=544), dict(D=0),
               dict(cap=0), dict(row0=-1), dict(row0=13), dict(n=17), dict(ld=511), dict(gal=0x2004)):
        assert _enrol(L, **kw) == -22, kw
    for kw in (dict(q=None), dict(gal=None), dict(scores=None), dict(rows=None), dict(ws=None), dict(Q=0),
               dict(G=0), dict(G=2**31 - 1), dict(k=0), dict(k=9), dict(D=48), dict(D=544), dict(ld=500),
               dict(labels=0x5000), dict(ident=0x6000), dict(gal=0x2008), dict(ws=0x10010), dict(ws_bytes=0)):
        assert _topk(L, **kw) == -22, kw
    need = L.prpe_gallery_topk_workspace_bytes(2, 100, 5)
    assert need > 0 and _topk(L, ws_bytes=need - 1) == -22                       # one byte short
    for Q, G, k in ((0, 10, 1), (1, 0, 1), (1, 10, 0), (1, 10, 9), (1, 2**31 - 1, 1)):
        assert L.prpe_gallery_topk_workspace_bytes(Q, G, k) == -22, (Q, G, k)


def test_gallery_plan_restates_the_library_plan():
    from prpe import ops
    L = _lib.lib()

    def a256(v):
        return (v + 255) // 256 * 256

    for Q in (1, 16, 17, 64, 65, 130, 256, 5000):
        for G in (1, 63, 64, 65, 4099, 70000, 1_000_000, 40_000_000):
            for k in (1, 8):
                qb, nqb, chunk, nchunks = ops.gallery_plan(Q, G)
                assert chunk % ops.GALLERY_STEP_ROWS == 0 and (nchunks - 1) * chunk < G <= nchunks * chunk
                assert qb * nqb >= Q > qb * (nqb - 1)
                assert L.prpe_gallery_topk_workspace_bytes(Q, G, k) == a256(Q * 512 * 4) + a256(nchunks * Q * k * 8)


# ---------------------------------------------------------------------------------- the rule
def _unit(*rows):
    return torch.tensor(rows, dtype=torch.float32)


def test_ref_exact_tie_takes_the_lower_row():
    g = _unit([0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [2, 0, 0, 0], [1, 0, 0, 0])   # rows 1, 3, 4 are one direction
    s, r = gallery_topk_ref(_unit([3, 0, 0, 0]), g, 4)
    assert r.tolist() == [[1, 3, 4, 0]] and s.tolist() == [[1.0, 1.0, 1.0, 0.0]]


def test_ref_fewer_rows_than_k_pads_with_minus_one():
    s, r = gallery_topk_ref(_unit([1, 1]), _unit([1, 0], [0, -1]), 5)
    assert r.tolist() == [[0, 1, -1, -1, -1]]
    assert s[0, :2].tolist() == pytest.approx([2 ** -0.5, -2 ** -0.5]) and torch.isneginf(s[0, 2:]).all()


def test_ref_nan_rows_and_masked_rows_are_skipped():
    g = _unit([1, 0], [float("nan"), 1], [0.6, 0.8], [0, 1])
    s, r = gallery_topk_ref(_unit([0, 1], [float("nan"), 0]), g, 3, valid=torch.tensor([1, 1, 1, 0], dtype=torch.uint8))
    assert r.tolist() == [[2, 0, -1], [-1, -1, -1]]          # row 1 is NaN, row 3 masked; a NaN query matches nothing
    assert s[0, :2].tolist() == pytest.approx([0.8, 0.0]) and torch.isneginf(s[1]).all()
    # a zero query scores 0 against every row: rows in ascending order
    s, r = gallery_topk_ref(_unit([0, 0]), g, 3)
    assert r.tolist() == [[0, 2, 3]] and s.tolist() == [[0.0, 0.0, 0.0]]


def test_ref_threshold_edge_is_inclusive():
    g = _unit([0.6, 0.8], [1, 0])
    labels = torch.tensor([2 ** 40 + 7, 5])
    q = _unit([0, 1])
    top = float(gallery_topk_ref(q, g, 1)[0][0, 0])
    below, above = float(torch.nextafter(torch.tensor(top, dtype=torch.float64), torch.tensor(-1.0, dtype=torch.float64))), \
        float(torch.nextafter(torch.tensor(top, dtype=torch.float64), torch.tensor(2.0, dtype=torch.float64)))
    assert gallery_topk_ref(q, g, 1, labels=labels, threshold=top)[2].tolist() == [2 ** 40 + 7]
    assert gallery_topk_ref(q, g, 1, labels=labels, threshold=below)[2].tolist() == [2 ** 40 + 7]
    assert gallery_topk_ref(q, g, 1, labels=labels, threshold=above)[2].tolist() == [-1]
    # no valid row at all: -1 whatever the threshold
    none = gallery_topk_ref(q, g, 1, valid=torch.zeros(2, dtype=torch.uint8), labels=labels, threshold=-2.0)
    assert none[1].tolist() == [[-1]] and none[2].tolist() == [-1]


# ---------------------------------------------------------------------------------- FaceGallery
class _Stub:
    """The two ops calls FaceGallery makes, recorded; topk answers row 0 for every query."""

    def __init__(self):
        self.enrol, self.topk = [], []

    def gallery_enrol(self, x, gallery, norms, row0=0):
        self.enrol.append((tuple(x.shape), int(row0)))

    def gallery_topk(self, q, gallery, G, k, *, scores, rows, valid=None, labels=None, threshold=0.0, ident=None,
                     workspace=None):
        self.topk.append((tuple(q.shape), G, k, threshold))
        scores.fill_(1.0)
        rows.zero_()
        if ident is not None:
            ident.copy_(labels[rows[:, 0].long()])


@pytest.fixture()
def gallery(monkeypatch):
    import prpe
    from prpe import gallery as gmod
    stub = _Stub()
    monkeypatch.setattr(gmod.ops, "gallery_enrol", stub.gallery_enrol)
    monkeypatch.setattr(gmod.ops, "gallery_topk", stub.gallery_topk)
    # the bookkeeping is host logic and elementwise torch ops: run it on CPU tensors
    monkeypatch.setattr(prpe.FaceGallery, "_embeddings", lambda self, what, e: e.float().contiguous())
    g = prpe.FaceGallery(dim=64, capacity=8, device="cpu")
    g.stub = stub
    return g


def test_gallery_is_exported_and_validates_its_shape():
    import prpe
    assert "FaceGallery" in prpe.__all__ and "FaceIdentifier" in prpe.__all__
    for kw in (dict(dim=48), dict(dim=544), dict(dim=16), dict(capacity=0)):
        with pytest.raises(ValueError):
            prpe.FaceGallery(device="cpu", **{**dict(dim=64, capacity=4), **kw})


def test_gallery_add_appends_and_overflow_leaves_the_state_unchanged(gallery):
    g = gallery
    assert len(g) == 0
    assert g.add(torch.ones(3, 64), [10, 11, 2 ** 40]) == (0, 3)
    assert g.add(torch.ones(2, 64), torch.tensor([12, 10])) == (3, 5)
    assert len(g) == 5 and g.stub.enrol == [((3, 64), 0), ((2, 64), 3)]
    assert g.labels[:5].tolist() == [10, 11, 2 ** 40, 12, 10] and g.valid.tolist() == [1] * 5 + [0] * 3
    before = (g.labels.clone(), g.valid.clone(), len(g), list(g.stub.enrol))
    with pytest.raises(ValueError, match="capacity"):
        g.add(torch.ones(4, 64), [1, 2, 3, 4])
    with pytest.raises(ValueError, match="labels"):
        g.add(torch.ones(2, 64), [1])
    assert torch.equal(g.labels, before[0]) and torch.equal(g.valid, before[1]) and len(g) == before[2]
    assert g.stub.enrol == before[3]                                   # nothing was launched either
    assert g.add(torch.ones(3, 64), [20, 21, 22]) == (5, 8) and len(g) == 8      # exactly full is fine


def test_gallery_remove_clears_valid_and_keeps_the_rows_in_place(gallery):
    g = gallery
    g.add(torch.ones(5, 64), [10, 11, 12, 10, 13])
    g.remove([10, 99])
    assert g.valid.tolist() == [0, 1, 1, 0, 1, 0, 0, 0] and len(g) == 5
    g.remove(torch.tensor([13]))
    assert g.valid.tolist() == [0, 1, 1, 0, 0, 0, 0, 0]
    g.remove([])
    assert g.valid.tolist() == [0, 1, 1, 0, 0, 0, 0, 0]
    assert g.add(torch.ones(1, 64), [10]) == (5, 6)                    # a removed label can be enrolled again
    assert g.valid.tolist() == [0, 1, 1, 0, 0, 1, 0, 0]


def test_gallery_search_identify_and_reset(gallery):
    g = gallery
    with pytest.raises(ValueError, match="empty"):
        g.search(torch.ones(1, 64))
    g.add(torch.ones(2, 64), [2 ** 33 + 1, 4])
    s, r, lab = g.search(torch.ones(3, 64), k=2)
    assert s.shape == (3, 2) and r.dtype == torch.int32 and lab.tolist() == [[2 ** 33 + 1] * 2] * 3
    ident, score = g.identify(torch.ones(3, 64), 0.5)
    assert ident.tolist() == [2 ** 33 + 1] * 3 and score.shape == (3,)
    assert g.stub.topk == [((3, 64), 2, 2, 0.0), ((3, 64), 2, 1, 0.5)]   # G = the enrolled rows, not the capacity
    g.reset()
    assert len(g) == 0 and g.valid.sum() == 0 and (g.labels == -1).all()
    with pytest.raises(ValueError, match="empty"):
        g.identify(torch.ones(1, 64), 0.5)
