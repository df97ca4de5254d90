"""CPU: the wide-batch gallery search (csrc/gallery_wide.hip) -- the proven bound
eps(D) between the bf16 filter's scores and the exact chain's, the filter rule restated on the host
(twice: tensor operations and a plain loop), the superset property it promises, the "auto"
dispatch and the argument checks. tests/test_gpu_gallery_wide.py imports the restatement.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from prpe import _lib, ops

NEG = float("-inf")
POS = float("inf")
L, C = ops.GALLERY_WIDE_L, ops.GALLERY_WIDE_C


# ---------------------------------------------------------------------------------- restatements
def coarse_scores(qn, gn):
    """The filter's scores [Q, G] of normalised fp32 rows: both sides rounded to bf16 (nearest even),
    products and sums in fp32 (the summation order is the host's; the tests leave 8 D 2^-24 for it)."""
    return qn.to(torch.bfloat16).float() @ gn.to(torch.bfloat16).float().t()


def chain_scores(qn, gn):
    """The exact route's scores [Q, G]: (a0 + a1) + (a2 + a3), a_e = fma(g[c], q[c], a_e) over the
    columns c = e mod 4 ascending. The fma is a product and a sum in fp64 rounded to fp32 (the
    product of two fp32 is exact in fp64)."""
    Q, D = qn.shape
    acc = [torch.zeros(Q, gn.shape[0]) for _ in range(4)]
    q64, g64 = qn.double(), gn.double()
    for c in range(D):
        acc[c % 4] = (q64[:, c:c + 1] * g64[:, c].unsqueeze(0) + acc[c % 4].double()).float()
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def filter_rule(coarse, k, chunk, eps, valid=None):
    """One query's certificate by the stated rule, in tensor operations. coarse [G] fp32 (a score
    that is not finite orders as +inf; rows with a zero valid byte never enter). Per chunk of
    ``chunk`` rows: the L best (score descending, row ascending) and spill, the largest score left
    out (-inf if none). t = the k-th largest finite listed score (-inf with fewer), bar = t - 2 eps
    in fp32. Candidates: the listed entries >= bar. Returns (certified, candidate rows, margin):
    certified = at most C candidates and every spill either -inf or < bar; margin = how far the
    nearest of those conditions is from flipping (positive when certified)."""
    G = coarse.shape[0]
    s = torch.where(torch.isfinite(coarse), coarse, torch.full_like(coarse, POS))
    if valid is not None:
        s = torch.where(valid[:G] != 0, s, torch.full_like(s, NEG))          # -inf: absent (no present row has it)
    nchunks = -(-G // chunk)
    pad = torch.full((nchunks * chunk,), NEG)
    pad[:G] = s
    top, idx = torch.sort(pad.view(nchunks, chunk), dim=1, descending=True, stable=True)
    listed, spill = top[:, :L], (top[:, L] if chunk > L else torch.full((nchunks,), NEG))
    rows = (idx[:, :L] + torch.arange(nchunks).unsqueeze(1) * chunk)[listed > NEG]
    listed = listed[listed > NEG]
    finite = torch.sort(listed[listed < POS], descending=True).values
    t = finite[k - 1] if finite.numel() >= k else torch.tensor(NEG)
    bar = (t - torch.tensor(2 * eps, dtype=torch.float32)).float()
    cand = rows[listed >= bar]
    dropped = spill[spill > NEG]
    certified = cand.numel() <= C and bool((dropped < bar).all())
    order = torch.sort(listed, descending=True).values
    m = float(bar - order[C]) if order.numel() > C else POS
    if dropped.numel():
        m = min(m, float(bar - dropped.max()))
    return certified, cand, m


def filter_rule_loop(coarse, k, chunk, eps, valid=None):
    """The same rule as a plain loop over rows (no sort of tensors, no shared code)."""
    G = len(coarse)
    lists, spills = [], []
    for r0 in range(0, G, chunk):
        best, spill = [], NEG
        for row in range(r0, min(r0 + chunk, G)):
            if valid is not None and int(valid[row]) == 0:
                continue
            v = float(coarse[row])
            v = v if v == v and abs(v) != POS else POS
            best.append((-v, row))
            best.sort()
            if len(best) > L:
                spill = max(spill, -best.pop()[0])
        lists += best
        spills.append(spill)
    finite = sorted((-s for s, _ in lists if -s < POS), reverse=True)
    t = finite[k - 1] if len(finite) >= k else NEG
    bar = float(torch.tensor(t, dtype=torch.float32) - torch.tensor(2 * eps, dtype=torch.float32))
    cand = [row for s, row in lists if -s >= bar]
    certified = len(cand) <= C and all(sp == NEG or sp < bar for sp in spills)
    return certified, cand


def exact_topk_rows(s64, k, valid=None):
    """The rows of the fp64 top-k (score descending, row ascending), non-finite and invalid skipped."""
    s = torch.where(torch.isfinite(s64), s64, torch.full_like(s64, NEG))
    if valid is not None:
        s = torch.where(valid != 0, s, torch.full_like(s, NEG))
    top, rows = torch.sort(s, descending=True, stable=True)
    return [int(r) for v, r in zip(top[:k], rows[:k]) if v > NEG]


# ---------------------------------------------------------------------------------- eps
def _midpoint_below(v):
    """The largest bf16 rounding midpoint (an odd multiple of half a bf16 ulp) not above v > 0."""
    e = torch.floor(torch.log2(torch.tensor(float(v), dtype=torch.float64)))
    half_ulp = 2.0 ** (float(e) - 8)
    m = int(v / half_ulp)
    m -= 1 - m % 2
    return m * half_ulp


def _adversarial(D):
    g = torch.Generator().manual_seed(D)
    mid = _midpoint_below(D ** -0.5)
    assert float(torch.tensor(mid).to(torch.bfloat16)) != mid and mid * D ** 0.5 <= 1.0
    aligned = torch.full((1, D), mid)
    signs = torch.where(torch.rand(6, D, generator=g) < 0.5, -1.0, 1.0)
    big = torch.zeros(3, D)
    big[0, 0] = _midpoint_below(1.0)
    big[1, D - 1] = -_midpoint_below(1.0)
    big[2, 0], big[2, 1:] = _midpoint_below(0.9), _midpoint_below((0.18 / (D - 1)) ** 0.5)
    rows = torch.cat([aligned, -aligned, aligned * signs, big]).float()
    assert float(rows.double().norm(dim=1).max()) <= 1.0
    return rows


@pytest.mark.parametrize("D", [32, 96, 512])
def test_eps_bounds_the_filter_and_the_chain_against_fp64(D):
    assert ops.gallery_wide_eps(D) == 2.0 ** -7 + 2.0 ** -16 + D * 2.0 ** -22
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    macro = re.search(r"#define PRPE_GALLERY_WIDE_EPS\(D\) (.*)", header).group(1)
    assert eval(macro.replace("(double)", ""), {"D": D}) == ops.gallery_wide_eps(D)
    g = torch.Generator().manual_seed(100 + D)
    unit = F.normalize(torch.randn(48, D, generator=g), dim=1)
    near = F.normalize(unit[:16] + 0.05 * torch.randn(16, D, generator=g) / D ** 0.5, dim=1)
    adv = _adversarial(D)
    worst = 0.0
    for qn, gn in ((unit[:24], torch.cat([unit[24:], near, unit[:8]])), (adv, adv), (adv, torch.cat([unit[:8], near]))):
        s64 = qn.double() @ gn.double().t()
        err = (coarse_scores(qn, gn).double() - s64).abs() + (chain_scores(qn, gn).double() - s64).abs()
        worst = max(worst, float(err.max()))
    print(f"gallery wide eps D={D}: worst |coarse - fp64| + |chain - fp64| = {worst:.6f}, eps = {ops.gallery_wide_eps(D):.6f}")
    assert worst <= ops.gallery_wide_eps(D)


# ---------------------------------------------------------------------------------- superset
def _datasets():
    g = torch.Generator().manual_seed(9)
    D, G = 64, 1500
    rand = F.normalize(torch.randn(G, D, generator=g), dim=1)
    dup = rand.clone()
    dup[torch.randint(0, G, (600,), generator=g)] = rand[torch.randint(0, 20, (600,), generator=g)]
    centres = F.normalize(torch.randn(12, D, generator=g), dim=1)
    clustered = F.normalize(centres[torch.randint(0, 12, (G,), generator=g)] +
                            0.25 * torch.randn(G, D, generator=g) / D ** 0.5, dim=1)
    out = {}
    for name, gal in (("random", rand), ("duplicates", dup), ("clustered", clustered)):
        q = F.normalize(torch.cat([gal[:12] + 0.3 * torch.randn(12, D, generator=g) / D ** 0.5,
                                   torch.randn(6, D, generator=g)]), dim=1)
        out[name] = (q, gal)
    return out


@pytest.mark.parametrize("name", ["random", "duplicates", "clustered"])
def test_certified_candidates_contain_the_fp64_topk(name):
    qn, gn = _datasets()[name]
    G, D = gn.shape
    valid = (torch.rand(G, generator=torch.Generator().manual_seed(1)) < 0.9).to(torch.uint8)
    coarse, s64 = coarse_scores(qn, gn), qn.double() @ gn.double().t()
    ncert = 0
    for chunk in (64, 128):
        for k in (1, 5, 8):
            for v in (None, valid):
                for i in range(qn.shape[0]):
                    cert, cand, margin = filter_rule(coarse[i], k, chunk, ops.gallery_wide_eps(D), v)
                    cert2, cand2 = filter_rule_loop(coarse[i], k, chunk, ops.gallery_wide_eps(D), v)
                    assert cert == cert2 and sorted(cand.tolist()) == sorted(cand2)      # the two statements agree
                    assert (margin > 0) == cert
                    if cert:
                        ncert += 1
                        assert set(exact_topk_rows(s64[i], k, v)) <= set(cand.tolist())
    print(f"gallery wide superset {name}: {ncert} certified of {2 * 3 * 2 * qn.shape[0]}")
    assert ncert > 0


def test_rule_keeps_non_finite_scores_and_counts_only_finite_ones_towards_t():
    coarse = torch.tensor([0.9, float("nan"), 0.5, float("inf"), 0.1, 0.89])
    cert, cand, _ = filter_rule(coarse, 1, 64, 0.008)
    assert cert and sorted(cand.tolist()) == [0, 1, 3, 5]                    # t = 0.9, not +inf
    assert filter_rule_loop(coarse, 1, 64, 0.008) == (True, [1, 3, 0, 5]) or \
        sorted(filter_rule_loop(coarse, 1, 64, 0.008)[1]) == [0, 1, 3, 5]
    cert, cand, _ = filter_rule(coarse, 8, 64, 0.008)                        # fewer than k: everything, nothing dropped
    assert cert and sorted(cand.tolist()) == [0, 1, 2, 3, 4, 5]
    many = torch.full((40,), float("nan"))
    assert not filter_rule(many, 1, 64, 0.008)[0] and not filter_rule_loop(many, 1, 64, 0.008)[0]   # +inf dropped


# ---------------------------------------------------------------------------------- ABI, dispatch, checks
def test_abi_has_the_wide_entry_points_and_refuses_bad_arguments():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    for res, name, nargs in (("int64_t", "prpe_gallery_topk_wide_workspace_bytes", 3), ("int", "prpe_gallery_topk_wide", 17)):
        decl = re.search(r"\b" + res + " " + name + r"\s*\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.lib(), name)
    Lb = _lib.lib()

    def call(q=0x1000, ld=512, Q=2, D=512, gal=0x2000, G=100, valid=None, k=5, scores=0x3000, rows=0x4000,
             labels=None, thr=0.0, ident=None, route=None, ws=0x10000, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = Lb.prpe_gallery_topk_wide_workspace_bytes(Q, G, min(max(k, 1), 8))
        return Lb.prpe_gallery_topk_wide(q, ld, Q, D, gal, G, valid, k, scores, rows, labels, thr, ident, route, ws,
                                         ws_bytes, None)

    for kw in (dict(q=None), dict(gal=None), dict(scores=None), dict(rows=None), dict(ws=None), dict(Q=0),
               dict(G=0), dict(G=2**31 - 1), dict(k=0), dict(k=9), dict(D=48), dict(D=544), dict(ld=500),
               dict(labels=0x5000), dict(ident=0x6000), dict(gal=0x2008), dict(ws=0x10010), dict(ws_bytes=0)):
        assert call(**kw) == -22, kw
    need = Lb.prpe_gallery_topk_wide_workspace_bytes(2, 100, 5)
    assert need > Lb.prpe_gallery_topk_workspace_bytes(2, 100, 5) and call(ws_bytes=need - 1) == -22
    for Q, G, k in ((0, 10, 1), (1, 0, 1), (1, 10, 0), (1, 10, 9), (1, 2**31 - 1, 1)):
        assert Lb.prpe_gallery_topk_wide_workspace_bytes(Q, G, k) == -22, (Q, G, k)


def test_wide_plan_covers_the_gallery():
    for Q in (1, 64, 65, 300, 2048, 5000):
        for G in (1, 63, 64, 65, 4099, 32835, 1_000_000, 40_000_000):
            nqb, chunk, nchunks = ops.gallery_wide_plan(Q, G)
            assert chunk % ops.GALLERY_STEP_ROWS == 0 and (nchunks - 1) * chunk < G <= nchunks * chunk
            assert ops.GALLERY_WIDE_QB * nqb >= Q > ops.GALLERY_WIDE_QB * (nqb - 1)


def test_auto_dispatch_and_route_names():
    m, n = ops.GALLERY_WIDE_MIN_Q, ops.GALLERY_WIDE_MIN_G
    assert ops.gallery_route("exact", 10 ** 6, 10 ** 7) == "exact" and ops.gallery_route("wide", 1, 1) == "wide"
    assert ops.gallery_route("auto", m - 1, n) == "exact" and ops.gallery_route("auto", m, n) == "wide"
    assert ops.gallery_route("auto", 10 * m, n - 1) == "exact"
    for bad in ("fast", None, ""):
        with pytest.raises(ValueError):
            ops.gallery_route(bad, 4, 4)


class _Stub:
    def __init__(self):
        self.calls = []

    def exact(self, q, gallery, G, k, *, scores, rows, **kw):
        self.calls.append(("exact", q.shape[0], k))
        scores.fill_(1.0)
        rows.zero_()
        if kw.get("ident") is not None:
            kw["ident"].fill_(7)

    def wide(self, q, gallery, G, k, *, scores, rows, **kw):
        self.exact(q, gallery, G, k, scores=scores, rows=rows, **kw)
        self.calls[-1] = ("wide",) + self.calls[-1][1:]


def test_face_gallery_takes_the_route_it_is_given(monkeypatch):
    import prpe
    from prpe import gallery as gmod
    stub = _Stub()
    monkeypatch.setattr(gmod.ops, "gallery_enrol", lambda e, rows, norms, row0: None)
    monkeypatch.setattr(gmod.ops, "gallery_topk", stub.exact)
    monkeypatch.setattr(gmod.ops, "gallery_topk_wide", stub.wide)
    monkeypatch.setattr(prpe.FaceGallery, "_embeddings", lambda self, what, e: e.float().contiguous())
    m = ops.GALLERY_WIDE_MIN_Q
    monkeypatch.setattr(gmod.ops, "GALLERY_WIDE_MIN_G", 2)       # two enrolled rows are a large gallery here
    few, many = torch.ones(m - 1, 64), torch.ones(m, 64)
    for route, want in (("exact", ["exact"] * 4), ("wide", ["wide"] * 4), ("auto", ["exact", "exact", "wide", "wide"])):
        g = prpe.FaceGallery(dim=64, capacity=8, device="cpu", route=route)
        g.add(torch.ones(2, 64), [1, 2])
        stub.calls.clear()
        g.search(few, 2), g.identify(few, 0.5), g.search(many, 2), g.identify(many, 0.5)
        assert [c[0] for c in stub.calls] == want
        stub.calls.clear()
        g.search(few, 2, route="wide"), g.identify(many, 0.5, route="exact"), g.search(many, 2, route="auto")
        assert [c[0] for c in stub.calls] == ["wide", "exact", "wide"]
        with pytest.raises(ValueError):
            g.search(few, 2, route="fast")
    assert prpe.FaceGallery(dim=64, capacity=8, device="cpu").route == "exact"       # the default is today's route
    g = prpe.FaceGallery(dim=64, capacity=8, device="cpu", route="auto")
    g.add(torch.ones(1, 64), [1])
    stub.calls.clear()
    g.search(many, 1)
    assert [c[0] for c in stub.calls] == ["exact"]                                   # below the row bar: exact
    with pytest.raises(ValueError):
        prpe.FaceGallery(dim=64, capacity=8, device="cpu", route="fast")


def test_ops_wide_checks_its_arguments_before_the_library():
    q, gal = torch.zeros(4, 64), torch.zeros(10, 64)
    s, r = torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.int32)
    for kw in (dict(k=9), dict(G=11), dict(G=0)):
        with pytest.raises(ValueError, match="prpe_gallery_topk_wide"):
            ops.gallery_topk_wide(q, gal, kw.get("G", 10), kw.get("k", 5), scores=s, rows=r)
    with pytest.raises(ValueError):
        ops.gallery_topk_wide(torch.zeros(4, 48), torch.zeros(10, 48), 10, 5, scores=s, rows=r)
    with pytest.raises(ValueError):
        ops.gallery_topk_wide(q, gal, 10, 5, scores=s, rows=r)                  # host tensors
