"""GPU: the wide-batch gallery search (csrc/gallery_wide.hip) against the exact route.

prpe_gallery_topk_wide must write the bits prpe_gallery_topk writes: scores are compared with
torch.equal on their int32 views, rows and ident exactly. Which queries the bf16 filter certifies
(route 0) and which the exact kernels finish (route 1) is asserted where the host restatement of the
filter rule (tests/test_gallery_wide_host.py, on the device's own normalised rows) decides it with a
margin of 8 D 2^-24 -- more than the coarse scores can move with the accumulation order.

Outputs live in sentinel-filled guarded buffers (``Guarded``, tests/test_gpu_rowops.py).
"""
import ctypes as C
import functools

import pytest
import torch

from prpe import CombinedModel, FaceCrops, FaceGallery, ops
from prpe._lib import lib
from test_gallery_wide_host import coarse_scores, filter_rule
from test_gpu_rowops import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
ISENT = -7777
BSENT = 77


def _bits(t):
    return t.contiguous().view(torch.int32)


def enrol(x):
    """The device gallery [G, D] of host rows x."""
    gal = torch.empty(x.shape, device=DEV)
    ops.gallery_enrol(x.to(DEV).contiguous(), gal, torch.empty(x.shape[0], device=DEV), 0)
    return gal


def run(fn, q, gal, G, k, valid=None, labels=None, threshold=0.0, workspace=None):
    """One guarded launch of ops.gallery_topk or ops.gallery_topk_wide -> host
    (scores, rows, ident or None, route or None)."""
    Q = q.shape[0]
    wide = fn is ops.gallery_topk_wide
    s, r = Guarded((Q, k)), Guarded((Q, k), fill=ISENT, dtype=torch.int32)
    ident = Guarded((Q,), fill=ISENT, dtype=torch.int64) if labels is not None else None
    route = Guarded((Q,), fill=BSENT, dtype=torch.uint8) if wide else None
    kw = dict(route=route.view) if wide else {}
    fn(q.to(DEV), gal, G, k, scores=s.view, rows=r.view, valid=None if valid is None else valid.to(DEV),
       labels=None if labels is None else labels.to(DEV), threshold=threshold,
       ident=None if ident is None else ident.view, workspace=workspace, **kw)
    assert s.untouched() and r.untouched() and (ident is None or ident.untouched())
    assert route is None or route.untouched()
    return s.cpu(), r.cpu(), None if ident is None else ident.cpu(), None if route is None else route.cpu()


def both(q, gal, G, k, **kw):
    """Both routes on the same call; asserts equal bits and returns (exact outputs, route)."""
    es, er, ei, _ = run(ops.gallery_topk, q, gal, G, k, **kw)
    ws, wr, wi, route = run(ops.gallery_topk_wide, q, gal, G, k, **kw)
    assert torch.equal(_bits(ws), _bits(es))
    assert torch.equal(wr, er)
    assert (ei is None and wi is None) or torch.equal(wi, ei)
    assert bool(((route == 0) | (route == 1)).all())
    return es, er, ei, route


def make(Q, G, D, seed):
    """Rows and queries from one seeded generator; half the queries are a gallery row plus noise."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(G, D, generator=g)
    q = torch.randn(Q, D, generator=g)
    for i in range((Q + 1) // 2):
        q[i] = x[(i * 7) % G] + 0.3 * q[i]
    return q, x


@functools.lru_cache(maxsize=None)
def case(Q, G, D, seed=7):
    q, x = make(Q, G, D, seed)
    return q, enrol(x)


# Q: below a 64-query block, one block, one past it, several; G: below a 64-row chunk, one chunk, one
# past it, many chunks, off every multiple. Every (Q edge, G edge) pair occurs.
SHAPES = [(Q, G, (32, 96, 512)[(i + j) % 3], (1, 5, 8)[(i + 2 * j) % 3])
          for i, Q in enumerate((17, 64, 65)) for j, G in enumerate((5, 64, 65))]
SHAPES += [(1, 1, 32, 1), (1, 70, 512, 5), (1, 4099, 96, 8), (17, 1, 96, 8), (17, 1025, 512, 1), (64, 70, 96, 1),
           (64, 4099, 32, 5), (130, 5, 512, 8), (130, 1025, 96, 5), (130, 4099, 512, 8), (300, 1, 512, 5),
           (300, 70, 32, 8), (300, 1025, 32, 1), (300, 4099, 96, 5), (64, 32835, 512, 5)]


@pytest.mark.parametrize("Q,G,D,k", SHAPES)
def test_wide_route_has_the_exact_routes_bits(Q, G, D, k):
    q, gal = case(Q, G, D)
    labels = (torch.arange(G, dtype=torch.int64) * 3 + 2 ** 34)
    es, er, ei, route = both(q, gal, G, k, labels=labels, threshold=0.5)
    n = min(G, k)
    assert (er[:, n:] == -1).all() and torch.isneginf(es[:, n:]).all()
    print(f"wide Q={Q} G={G} D={D} k={k}: plan={ops.gallery_wide_plan(Q, G)} fallback share={float(route.float().mean()):.3f}")


def _variation(name):
    Q, G, D, k = 130, 1025, 96, 5
    q, x = make(Q, G, D, 11)
    q, x = q.clone(), x.clone()
    kw = {}
    if name == "valid_mask":
        kw["valid"] = (torch.rand(G, generator=torch.Generator().manual_seed(3)) < 0.6).to(torch.uint8)
        kw["valid"][(torch.arange(Q // 2) * 7) % G] = 0          # the planted best rows are masked out
    elif name == "all_invalid":
        kw["valid"] = torch.zeros(G, dtype=torch.uint8)
    elif name == "zero_query":
        q[0] = 0
        q[77] = 0
    elif name == "zero_row":
        x[0] = 0
        x[640] = 0
    elif name == "nonfinite_queries":
        q[3, 5] = float("nan")
        q[64, 0] = float("inf")
        q[129, 95] = float("-inf")
    elif name == "nonfinite_rows":
        x[7, 1] = float("nan")
        x[64] = float("nan")
    gal = enrol(x)
    if name == "nonfinite_rows":
        # elements written past the enrolment: an infinite and a NaN element in otherwise unit rows
        gal[14, 3] = float("inf")
        gal[128, 95] = float("-inf")
        gal[1024, 0] = float("nan")
    return q, gal, G, k, kw


@pytest.mark.parametrize("name", ["plain", "valid_mask", "all_invalid", "zero_query", "zero_row", "nonfinite_queries",
                                  "nonfinite_rows"])
def test_wide_route_variations_have_the_exact_routes_bits(name):
    q, gal, G, k, kw = _variation(name)
    labels = torch.arange(G, dtype=torch.int64) + 5
    es, er, ei, route = both(q, gal, G, k, labels=labels, threshold=0.3, **kw)
    if name == "all_invalid":
        assert (er == -1).all() and (ei == -1).all()
    if name == "nonfinite_queries":
        assert (er[[3, 64, 129]] == -1).all()
    if name == "nonfinite_rows":
        assert not any(int(v) in (7, 14, 64, 128, 1024) for v in er.reshape(-1))
    print(f"wide variation {name}: fallback share={float(route.float().mean()):.3f}")


def test_wide_route_fewer_rows_than_k():
    q, gal = case(65, 5, 96)
    es, er, _, _ = both(q, gal, 3, 8)
    assert (er[:, 3:] == -1).all() and (er[:, :3] >= 0).all()


def test_wide_route_threshold_at_exact_equality_with_the_best_score():
    q, gal = case(130, 1025, 96)
    G = 1025
    labels = torch.arange(G, dtype=torch.int64) + 100
    es, er, _, _ = run(ops.gallery_topk, q, gal, G, 1)
    for qi in (0, 64, 129):
        thr = float(es[qi, 0])
        _, _, ei, _ = both(q, gal, G, 1, labels=labels, threshold=thr)
        assert int(ei[qi]) == int(er[qi, 0]) + 100                           # equality accepts


def _call_wide(q, ld, Q, D, gal, G, valid, k, s, r, labels, thr, ident, route, ws, ws_bytes):
    p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    return lib().prpe_gallery_topk_wide(p(q), ld, Q, D, p(gal), G, p(valid), k, p(s), p(r), p(labels), thr, p(ident),
                                        p(route), p(ws), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_wide_route_strided_queries():
    Q, G, D, k = 130, 1025, 96, 5
    q, gal = case(Q, G, D)
    es, er, _, _ = run(ops.gallery_topk, q, gal, G, k)
    wide = Guarded((Q, D), stride=(D + 40, 1), fill=float("nan"))
    wide.view.copy_(q.to(DEV))
    s, r = Guarded((Q, k)), Guarded((Q, k), fill=ISENT, dtype=torch.int32)
    nbytes = lib().prpe_gallery_topk_wide_workspace_bytes(Q, G, k)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    assert _call_wide(wide.view, D + 40, Q, D, gal, G, None, k, s.view, r.view, None, 0.0, None, None, ws, nbytes) == 0
    assert s.untouched() and r.untouched()
    assert torch.equal(_bits(s.cpu()), _bits(es)) and torch.equal(r.cpu(), er)


def test_wide_route_exact_duplicates_tie_on_the_lower_row():
    Q, G, D, k = 65, 4099, 96, 8
    _, chunk, _ = ops.gallery_wide_plan(Q, G)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(G, D, generator=g)
    pos = sorted({0, 15, 16, 63, 64, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, 17 * chunk + 31, G - 1})
    for p in pos:
        x[p] = x[0]
    q = torch.randn(Q, D, generator=g)
    q[0] = x[0]
    q[64] = x[0] * 3
    es, er, _, route = both(q, enrol(x), G, k)
    for qi in (0, 64):
        assert er[qi].tolist() == pos[:k]
        assert len(set(_bits(es[qi]).tolist())) == 1                         # one score, bit for bit


# ---------------------------------------------------------------------------------- the certificate
def _margins(q, gal, G, k, valid=None):
    """The host restatement on the device's own normalised rows: (certified [Q], margin [Q])."""
    D = q.shape[1]
    qn = enrol(q).cpu()
    coarse = coarse_scores(qn, gal[:G].cpu())
    _, chunk, _ = ops.gallery_wide_plan(q.shape[0], G)
    out = [filter_rule(coarse[i], k, chunk, ops.gallery_wide_eps(D), valid) for i in range(q.shape[0])]
    return torch.tensor([o[0] for o in out]), torch.tensor([o[2] for o in out])


@functools.lru_cache(maxsize=None)
def planted(D=96, G=4099, Q=70):
    """Random unit rows with, per query i, neighbours planted at cosines 0.9, 0.8, 0.7, 0.6; identity A
    with 20 near-duplicates in consecutive rows of one chunk; identity B with 80 near-duplicates, 4 in
    each of 20 chunks."""
    g = torch.Generator().manual_seed(23)
    x = torch.nn.functional.normalize(torch.randn(G, D, generator=g), dim=1)
    _, chunk, nchunks = ops.gallery_wide_plan(Q, G)
    assert chunk == 64 and nchunks >= 60 and ops.gallery_wide_plan(300, G)[1] == chunk
    q = x[torch.arange(Q) * 3 + 1].clone()
    for i in range(Q):
        for j, cosine in enumerate((0.9, 0.8, 0.7, 0.6)):
            row = 3200 + 4 * i + j
            noise = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
            noise = torch.nn.functional.normalize(noise - (noise @ q[i]) * q[i], dim=0)
            x[row] = cosine * q[i] + (1 - cosine ** 2) ** 0.5 * noise
    a = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
    b = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
    near = lambda v: v + 0.02 * torch.randn(D, generator=g) / D ** 0.5
    for j in range(20):
        x[5 * chunk + 5 + j] = near(a)
    for ch in range(20):
        for j in range(4):
            x[(ch + 6) * chunk + 10 + 9 * j] = near(b)
    return q, x, enrol(x), a, b


MARGIN = lambda D: 8 * D * 2.0 ** -24


@pytest.mark.parametrize("k", [1, 5])
def test_planted_neighbours_are_certified(k):
    q, x, gal, _, _ = planted()
    G, D = x.shape
    cert, margin = _margins(q, gal, G, k)
    assert bool(cert.all()) and float(margin.min()) >= MARGIN(D)             # the host rule, with room
    es, er, _, route = both(q, gal, G, k)
    assert (route == 0).all()
    if k == 5:
        want = torch.tensor([[3 * i + 1] + [3200 + 4 * i + j for j in range(4)] for i in range(q.shape[0])])
        assert torch.equal(er.long(), want)


def test_near_duplicates_past_the_list_fall_back_and_the_others_do_not():
    q, x, gal, a, _ = planted()
    G, D = x.shape
    q = q.clone()
    q[9] = a
    cert, margin = _margins(q, gal, G, 8)
    assert not bool(cert[9]) and float(margin[9]) <= -MARGIN(D)              # the 9th best is within the bar
    others = torch.arange(q.shape[0]) != 9
    assert bool(cert[others].all()) and float(margin[others].min()) >= MARGIN(D)
    _, er, _, route = both(q, gal, G, 8)
    assert route.tolist() == [1 if i == 9 else 0 for i in range(q.shape[0])]
    _, chunk, _ = ops.gallery_wide_plan(q.shape[0], G)
    assert all(5 * chunk + 5 <= int(v) < 5 * chunk + 25 for v in er[9])


def test_more_candidates_than_the_exact_pass_takes_fall_back():
    q, x, gal, _, b = planted()
    G, D = x.shape
    q = q.clone()
    q[0] = b
    coarse = coarse_scores(enrol(q).cpu()[:1], gal.cpu())[0]
    _, chunk, _ = ops.gallery_wide_plan(q.shape[0], G)
    cert, cand, margin = filter_rule(coarse, 5, chunk, ops.gallery_wide_eps(D))
    assert not cert and cand.numel() > ops.GALLERY_WIDE_C and margin <= -MARGIN(D)
    _, _, _, route = both(q, gal, G, 5)
    assert int(route[0]) == 1 and (route[1:] == 0).all()


def test_every_query_falls_back():
    _, x, gal, a, _ = planted()
    G, D = x.shape
    g = torch.Generator().manual_seed(2)
    q = a + 0.01 * torch.randn(70, D, generator=g) / D ** 0.5
    cert, margin = _margins(q, gal, G, 8)
    assert not bool(cert.any()) and float(margin.max()) <= -MARGIN(D)
    _, _, _, route = both(q, gal, G, 8)
    assert (route == 1).all()


def test_fallbacks_at_the_block_edges_of_the_list():
    q70, x, gal, a, _ = planted()
    G, D = x.shape
    q = x[3480 + 2 * torch.arange(300)].clone()      # untouched random rows, each its own best match
    q[:70] = q70
    hit = [0, 63, 64, 299]
    q[hit] = a
    cert, margin = _margins(q, gal, G, 8)
    want = torch.zeros(300, dtype=torch.bool)
    want[hit] = True
    assert torch.equal(~cert, want) and float(margin.abs().min()) >= MARGIN(D)
    _, _, _, route = both(q, gal, G, 8)
    assert torch.equal(route.bool(), want)


# ---------------------------------------------------------------------------------- determinism, isolation
def test_two_runs_and_two_streams_give_the_same_bytes():
    q, x, gal, a, _ = planted()
    G = x.shape[0]
    q = q.clone()
    q[9] = a
    first = run(ops.gallery_topk_wide, q, gal, G, 8)
    again = run(ops.gallery_topk_wide, q, gal, G, 8)
    for u, v in zip(first, again):
        assert u is None or torch.equal(u.view(torch.uint8) if u.dtype != torch.uint8 else u,
                                        v.view(torch.uint8) if v.dtype != torch.uint8 else v)
    q2, gal2 = case(130, 1025, 96)
    want2 = run(ops.gallery_topk_wide, q2, gal2, 1025, 5)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = []
    for st, (qq, gg, G_, k_) in zip(streams, ((q, gal, G, 8), (q2, gal2, 1025, 5))):
        with torch.cuda.stream(st):
            got.append(run(ops.gallery_topk_wide, qq, gg, G_, k_))
    torch.cuda.synchronize()
    for want, have in zip((first, want2), got):
        assert torch.equal(_bits(have[0]), _bits(want[0])) and torch.equal(have[1], want[1])
        assert torch.equal(have[3], want[3])


def test_refusals_write_nothing():
    Q, G, D, k = 17, 70, 96, 5
    q, gal = case(Q, G, D)
    qd = q.to(DEV)
    labels = torch.arange(G, dtype=torch.int64, device=DEV)
    need = lib().prpe_gallery_topk_wide_workspace_bytes(Q, G, k)
    assert need > lib().prpe_gallery_topk_workspace_bytes(Q, G, k)
    ws = torch.empty(need + 256, device=DEV, dtype=torch.uint8)
    s, r = Guarded((Q, k)), Guarded((Q, k), fill=ISENT, dtype=torch.int32)
    ident, route = Guarded((Q,), fill=ISENT, dtype=torch.int64), Guarded((Q,), fill=BSENT, dtype=torch.uint8)
    base = dict(q=qd, ld=D, Q=Q, D=D, gal=gal, G=G, valid=None, k=k, s=s.view, r=r.view, labels=labels, thr=0.0,
                ident=ident.view, route=route.view, ws=ws, ws_bytes=need)
    bad = [dict(q=None), dict(gal=None), dict(s=None), dict(r=None), dict(ws=None), dict(Q=0), dict(G=0),
           dict(G=2 ** 31 - 1), dict(k=0), dict(k=9), dict(D=48), dict(D=544), dict(ld=D - 1), dict(labels=None),
           dict(ident=None), dict(gal=gal.data_ptr() + 8), dict(ws=ws.data_ptr() + 16), dict(ws_bytes=need - 1),
           dict(ws_bytes=lib().prpe_gallery_topk_workspace_bytes(Q, G, k))]
    for kw in bad:
        assert _call_wide(**{**base, **kw}) == -22, kw
    torch.cuda.synchronize()
    for gbuf in (s, r, ident, route):
        assert bool((gbuf.buf == gbuf.fill).all())
    assert _call_wide(**base) == 0


# ---------------------------------------------------------------------------------- FaceGallery, FaceCrops
def test_face_gallery_routes_agree(monkeypatch):
    monkeypatch.setattr(ops, "GALLERY_WIDE_MIN_G", 100)      # "auto" takes the wide route on this small gallery
    g = torch.Generator().manual_seed(4)
    x = torch.randn(500, 64, generator=g).to(DEV)
    labels = torch.arange(500) + 2 ** 33
    gals = {}
    for route in ("exact", "wide", "auto"):
        gals[route] = FaceGallery(dim=64, capacity=600, device=DEV, route=route)
        gals[route].add(x, labels)
        gals[route].remove([2 ** 33 + 3])
    for Q in (3, ops.GALLERY_WIDE_MIN_Q + 6):
        probes = (x[:Q] + 0.2 * torch.randn(Q, 64, generator=g).to(DEV))
        want = gals["exact"].search(probes, 5) + gals["exact"].identify(probes, 0.4)
        for route in ("wide", "auto"):
            got = gals[route].search(probes, 5) + gals[route].identify(probes, 0.4)
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want))
        got = gals["exact"].search(probes, 5, route="wide") + gals["exact"].identify(probes, 0.4, route="wide")
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        FaceGallery(dim=64, capacity=4, device=DEV, route="fast")


def test_face_crops_identify_the_same_people_on_the_wide_route(state_dict):
    import test_gpu_faces as GF
    model = CombinedModel(state_dict, device=DEV)
    x = GF._model_frames()
    dets, counts = GF._dets([[(*GF.BOX_A, 0.9), (50.0, 50.0, 52.0, 53.0, 0.8), (*GF.BOX_B, 0.7)],
                             [(*GF.BOX_C, 0.6), (*GF.BOX_D, 0.5)]])
    labels = [2 ** 35 + 1, 2 ** 35 + 2, 2 ** 35 + 3, 99]
    ex = torch.stack([x[0], x[0], x[1], x[1]])
    ed, ec = GF._dets([[(*GF.BOX_A, 0.9), (*GF.BOX_D, 0.3)], [(*GF.BOX_B, 0.7)], [(*GF.BOX_C, 0.6)], [(*GF.BOX_D, 0.2)]])
    outs = {}
    for route in ("exact", "wide"):
        gallery = FaceGallery(dim=512, capacity=8, device=DEV, route=route)
        faces = FaceCrops(model, gallery, threshold=0.5, **GF.KW)
        assert faces.enrol_detections(ex, ed, ec, labels) == [3]
        outs[route] = faces.from_detections(x, dets, counts)
    assert outs["exact"]["ident"].tolist()[:3] == labels[:3]
    assert torch.equal(outs["wide"]["ident"], outs["exact"]["ident"])
    assert torch.equal(_bits(outs["wide"]["score"]), _bits(outs["exact"]["score"]))
