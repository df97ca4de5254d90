"""GPU: the open-set 1:N identification evaluation (csrc/identeval.hip) --
prpe_ident_best, prpe_ident_rank, prpe_ident_finish, and ``IdentificationEval`` /
``FaceIdentifier.calibrate_fpir`` above them -- against the host restatements of
tests/test_identeval_host.py (``ident_eval_ref`` in loops, ``ident_eval_sorted`` through fp64 and a
sort, ``ident_eval_blocks`` for the walked sizes), where the inputs and the conditions that allow
equalities (exact scores, ties, margins) are built and asserted on the CPU.

Every output lives in a sentinel-filled buffer with guards on both sides (``Guarded``,
tests/test_gpu_rowops.py); every launch is followed by a check that the guards are untouched.
All comparisons with the restatement are equalities of bytes. Up to 2 x 3 tiles every workgroup
takes one tile; the walked case takes its sizes from the CU count (``walk_sizes``), three tiles per
workgroup at least.

Measured on an MI355X: see DESIGN.md §5p.
"""
import functools

import numpy as np
import pytest
import torch

from prpe import FaceGallery, FaceIdentifier, IdentificationEval, _lib, ops
from prpe.identification import identification_curve
from test_faceverif_host import TILE, four_halves, thresholds_ref, tiles_of, walk_sizes, walk_sizes_cross
from test_gpu_faceverif import enrol
from test_gpu_rowops import Guarded
from test_identeval_host import (FIELDS, PLANTED_TOL, R, call_finish, call_ident, exact_case, exact_scores,
                                 finish_refusals, ident_eval_blocks, ident_eval_ref, ident_refusals, planted_reference,
                                 same_outputs, tie_case, walk_case)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ISENT = -7777
PER_PROBE = ("mate_score", "mate_row", "non_score", "non_row", "rank")


# ---------------------------------------------------------------------------------- harness
class Outs:
    """Guarded outputs for M probes: the caller-zeroed ones zeroed, the written ones full of sentinels."""

    def __init__(self, M, nbins):
        z = lambda shape, dtype=torch.int64: Guarded(shape, fill=ISENT, dtype=dtype)
        self.M, self.nbins = M, nbins
        self.g = {"mate_key": z((M,)), "non_key": z((M,)), "skipped": z((1,)), "rank_minus_1": z((M,), torch.int32),
                  "hist": z((3, nbins)), "rank_hist": z((R + 1,)), "counts": z((4,)),
                  "mate_score": z((M,), torch.float32), "non_score": z((M,), torch.float32),
                  "mate_row": z((M,), torch.int32), "non_row": z((M,), torch.int32), "rank": z((M,), torch.int32)}
        for k in ("mate_key", "non_key", "skipped", "rank_minus_1", "hist", "rank_hist", "counts"):
            self.g[k].view.zero_()

    def v(self, k, lo=0, hi=None):
        return self.g[k].view[lo:hi]

    def host(self):
        torch.cuda.synchronize()
        assert all(g.untouched() for g in self.g.values())
        out = {k: g.cpu().numpy() for k, g in self.g.items()}
        for k in ("mate_key", "non_key"):
            out[k] = out[k].view(np.uint64)
        out["skipped"] = int(out["skipped"][0])
        return out


def _dev(t, dtype):
    return None if t is None else torch.as_tensor(np.asarray(t)).to(dtype).to(DEV)


def rows_dev(x):
    return x if isinstance(x, torch.Tensor) or x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def passes(out, a, la, b=None, lb=None, va=None, vb=None, b_row0=0, lo=0, hi=None, which=(1, 2)):
    """Pass 1 and / or 2 for the probes lo .. hi of ``out`` against ``b`` (None: self mode)."""
    a, b = rows_dev(a), rows_dev(b)
    kw = dict(a_valid=_dev(va, torch.uint8), b_valid=_dev(vb, torch.uint8), b_row0=b_row0)
    la, lb = _dev(la, torch.int64), _dev(lb, torch.int64)
    if 1 in which:
        ops.ident_best(a, la, b, lb, mate_key=out.v("mate_key", lo, hi), non_key=out.v("non_key", lo, hi),
                       skipped=out.v("skipped"), **kw)
    if 2 in which:
        ops.ident_rank(a, la, b, lb, mate_key=out.v("mate_key", lo, hi), rank_minus_1=out.v("rank_minus_1", lo, hi), **kw)


def finish(out, la, va=None, lo=0, hi=None):
    ops.ident_finish(_dev(la, torch.int64), a_valid=_dev(va, torch.uint8), mate_key=out.v("mate_key", lo, hi),
                     non_key=out.v("non_key", lo, hi), rank_minus_1=out.v("rank_minus_1", lo, hi), nbins=out.nbins,
                     hist=out.v("hist"), rank_hist=out.v("rank_hist"), counts=out.v("counts"),
                     **{k: out.v(k, lo, hi) for k in PER_PROBE})


def run(a, la, b=None, lb=None, va=None, vb=None, nbins=256):
    out = Outs(len(la), nbins)
    passes(out, a, la, b, lb, va, vb)
    finish(out, la, va)
    return out.host()


# ---------------------------------------------------------------------------------- 1. exact inputs
@pytest.mark.parametrize("D,nbins", [(32, 256), (96, 1024), (512, 4096)])
def test_exact_inputs_equal_the_restatement_cross(D, nbins):
    """130 x 257: 2 x 3 tiles, ragged on both sides. D = 96 has NaN and inf elements in two probes
    and two gallery rows: their combinations are skipped, a probe made of NaN has no candidate."""
    a, b, la, lb, va, vb = exact_case(130, 2 * TILE + 1, D, 300 + D, spoil=D == 96)
    want = ident_eval_ref(exact_scores(a, b), la, lb, va, vb, nbins)
    got = run(a, la, b, lb, va, vb, nbins)
    same_outputs(got, want)
    assert (want["skipped"] > 0) == (D == 96) and (want["counts"][3] > 0) == (D == 96)
    assert (want["rank"] > 1).any() and want["counts"][:3].min() > 0 and want["hist"].sum(axis=1).min() > 0


@pytest.mark.parametrize("D,nbins", [(32, 512), (96, 256), (512, 2048)])
def test_exact_inputs_equal_the_restatement_self(D, nbins):
    """257 rows, leave-one-out: the restatement removes the diagonal of the set against itself. A
    probe whose identity has a single row counts as non-mated."""
    x, _, la, _, va, _ = exact_case(2 * TILE + 1, 0, D, 400 + D, spoil=D == 96)
    want = ident_eval_ref(exact_scores(x, x), la, None, va, None, nbins, self_mode=True)
    got = run(x, la, va=va, nbins=nbins)
    same_outputs(got, want)
    on = (la >= 0) & (va != 0)
    singles = [i for i in np.flatnonzero(on) if ((la == la[i]) & on).sum() == 1]
    assert singles and (got["rank"][singles] == 0).all() and (got["mate_row"][singles] == -1).all()
    assert got["counts"][1] >= len(singles) and (got["rank"] > 1).any()
    assert (got["rank_hist"][R] > 0) == (D == 512)                             # ranks past R share the last slot


# ---------------------------------------------------------------------------------- 2. ties
def test_ties_follow_row_order():
    a, b, la, lb, va, vb, said = tie_case()
    want = ident_eval_ref(exact_scores(a, b), la, lb, va, vb, 256)
    got = run(a, la, b, lb, va, vb, 256)
    same_outputs(got, want)
    for k, v in said.items():
        np.testing.assert_array_equal(got[k], np.asarray(v, dtype=got[k].dtype), err_msg=k)


# ---------------------------------------------------------------------------------- 3. the search's answers
def test_agreement_with_identify_and_search():
    """Raw probes are normalised by the search exactly as ``enrol`` normalises them
    (tests/test_gpu_faceverif.py), so the scores compared here have the same bits."""
    D, nbins = 96, 1024
    g = torch.Generator().manual_seed(71)
    ids = torch.arange(12).repeat_interleave(5)
    x = torch.randn(12, D, generator=g)[ids] + 3.5 * torch.randn(60, D, generator=g)
    q = torch.arange(60) % 5 < 3                                               # 3 rows of an identity enrolled, 2 probes
    y = torch.cat([x[~q], torch.randn(20, D, generator=g)])
    ly = torch.cat([ids[~q], 100 + torch.arange(20)]).numpy()
    gal = FaceGallery(dim=D, capacity=64, device=DEV)
    gal.add(x[q].to(DEV), ids[q])
    gal.remove([11])                                                           # identity 11's probes become strangers
    n = len(gal)
    got = run(enrol(y), ly, gal.rows[:n], gal.labels[:n].cpu().numpy(), vb=gal.valid[:n].cpu().numpy(), nbins=nbins)
    mated, stranger = got["rank"] > 0, (got["rank"] == 0)
    assert got["counts"].tolist() == [22, 22, 0, 0] and mated.sum() == 22 and (got["rank"] > 1).sum() >= 3 and (got["rank"] > 8).any()
    ident, best = gal.identify(y.to(DEV), -1.0)
    ident, best = ident.cpu().numpy(), best.cpu().numpy()
    np.testing.assert_array_equal((got["mate_key"] > got["non_key"]), ident == ly)
    np.testing.assert_array_equal(best, np.maximum(got["mate_score"], got["non_score"]))
    sc, rows, lab = gal.search(y.to(DEV), k=8)
    rows, lab = rows.cpu().numpy(), lab.cpu().numpy()
    for i in range(len(ly)):
        first = np.flatnonzero(lab[i] == ly[i])[:1]
        if 0 < got["rank"][i] <= 8:
            assert first.size and first[0] + 1 == got["rank"][i] and rows[i, first[0]] == got["mate_row"][i], i
        else:
            assert not first.size, i
    edges = thresholds_ref(nbins)
    at = sorted({int(np.searchsorted(edges, float(v), side="right")) - 1 for v in np.sort(best)[[3, 20, 40]]})
    assert len(at) == 3
    names_at_edges(gal, y.to(DEV), ly, got, at, nbins)
    # scores ON the edges: rows of four halves (the search leaves them as they are), every score a
    # multiple of 0.25 and so an edge of every nbins; >= includes them
    a, b, la, lb, va, vb = exact_case(40, 90, 32, 123)
    lb = np.abs(lb)
    gal = FaceGallery(dim=32, capacity=90, device=DEV)
    gal.add(torch.from_numpy(b).to(DEV), lb)
    gal.valid[:90] = torch.from_numpy(vb).to(DEV)
    assert torch.equal(gal.rows.cpu(), torch.from_numpy(b))
    got = run(a, la, b, lb, va, vb, 256)
    assert got["counts"][:3].min() > 0
    names_at_edges(gal, torch.from_numpy(a).to(DEV), la, got, [128 + 32, 128 + 64, 128 + 96, 255], 256, (la >= 0) & (va != 0))


def names_at_edges(gal, probes, labels, got, bins, nbins, part=None):
    """The sums of ``got["hist"]`` over the bins >= b against the right, wrong and stranger names
    ``gal.identify`` returns at threshold edge_b, for the probes that take part."""
    part = np.ones(len(labels), dtype=bool) if part is None else part
    mated, stranger = part & (got["rank"] > 0), part & (got["rank"] == 0)
    edges, totals = thresholds_ref(nbins), []
    for b in bins:
        named, _ = gal.identify(probes, float(edges[b]))
        named = named.cpu().numpy()
        want = [int((mated & (named == labels)).sum()), int((mated & (named >= 0) & (named != labels)).sum()),
                int((stranger & (named >= 0)).sum())]
        assert got["hist"][:, b:].sum(axis=1).tolist() == want, (b, want)
        totals.append(sum(want))
    assert totals[0] > 0 and totals == sorted(totals, reverse=True)


# ---------------------------------------------------------------------------------- 4. taking part
def test_a_probe_with_no_candidate_at_all_and_nothing_taking_part():
    x = four_halves(6, 32, 9)
    la = np.array([1, 1, -1], dtype=np.int64)
    want = ident_eval_ref(exact_scores(x[:3], x[3:]), la, [1, 2, 3], [1, 0, 1], [0, 0, 0], 256)
    got = run(x[:3], la, x[3:], [1, 2, 3], [1, 0, 1], [0, 0, 0])
    same_outputs(got, want)
    assert got["counts"].tolist() == [0, 1, 2, 1] and got["hist"].sum() == 0
    # self mode on one row is legal and finds nothing
    got = run(x[:1], [4])
    assert got["counts"].tolist() == [0, 1, 0, 1] and got["rank"].tolist() == [0] and got["skipped"] == 0


# ---------------------------------------------------------------------------------- 5. decomposition
def test_probes_in_two_calls_and_the_gallery_in_two_ranges_give_one_calls_numbers():
    M, N, nbins = TILE + 30, 2 * TILE + 1, 512
    a, b, la, lb, va, vb = exact_case(M, N, 32, 77)
    whole = run(a, la, b, lb, va, vb, nbins)
    same_outputs(whole, ident_eval_ref(exact_scores(a, b), la, lb, va, vb, nbins))
    for cut in (1, TILE + 1):                                                  # the probes split: views of every per-probe array
        out = Outs(M, nbins)
        for lo, hi in ((0, cut), (cut, M)):
            passes(out, a[lo:hi], la[lo:hi], b, lb, va[lo:hi], vb, lo=lo, hi=hi)
            finish(out, la[lo:hi], va[lo:hi], lo, hi)
        same_outputs(out.host(), whole)
    for cut in (TILE - 1, TILE + 60):                                          # the gallery split: b_row0 names the rows
        out = Outs(M, nbins)
        for which in ((1,), (2,)):                                             # pass 2 needs the whole gallery's mate_key
            for lo, hi in ((cut, N), (0, cut)):
                passes(out, a, la, b[lo:hi], lb[lo:hi], va, vb[lo:hi], b_row0=lo, which=which)
        finish(out, la, va)
        same_outputs(out.host(), whole)


# ---------------------------------------------------------------------------------- 6. strides, determinism
def test_strided_operands_with_nan_padding_and_two_runs_give_the_same_bits():
    M, N, D = 70, TILE + 9, 96
    a, b, la, lb, va, vb = exact_case(M, N, D, 91)
    want = run(a, la, b, lb, va, vb)
    wa = Guarded((M, D), stride=(D + 8, 1), fill=float("nan"))
    wb = Guarded((N, D), stride=(D + 4, 1), fill=float("nan"))
    wa.view.copy_(torch.from_numpy(a))
    wb.view.copy_(torch.from_numpy(b))
    assert wa.view.data_ptr() % 16 == 0 and wb.view.data_ptr() % 16 == 0
    same_outputs(run(wa.view, la, wb.view, lb, va, vb), want)
    same_outputs(run(wb.view, lb, va=vb), run(b, lb, va=vb))
    # random rows: whichever workgroup's maximum arrives first, the bits are the same
    rows = enrol(torch.randn(3 * TILE + 5, 64, generator=torch.Generator().manual_seed(5)))
    labels = np.arange(3 * TILE + 5) % 37
    one, two = run(rows, labels), run(rows, labels)
    for k in FIELDS:
        assert np.asarray(one[k]).tobytes() == np.asarray(two[k]).tobytes(), k
    assert (one["rank"] > 1).sum() > 50


# ---------------------------------------------------------------------------------- 7. refusals
def test_refusals_launch_nothing_and_write_nothing():
    L = _lib.lib()
    M = 100
    a, la = torch.zeros(M, 512, device=DEV), torch.zeros(M, dtype=torch.int64, device=DEV)
    out = Outs(M, 2048)
    p = lambda k: out.v(k).data_ptr()
    real = dict(a=a.data_ptr(), la=la.data_ptr(), mate=p("mate_key"), non=p("non_key"), skipped=p("skipped"),
                rm1=p("rank_minus_1"))
    for kw in ident_refusals():
        assert call_ident(L, "best", **{**real, **kw}) == -22 and call_ident(L, "rank", **{**real, **kw}) == -22, kw
    fin = dict(la=la.data_ptr(), mate=p("mate_key"), non=p("non_key"), rm1=p("rank_minus_1"), ms=p("mate_score"),
               mr=p("mate_row"), ns=p("non_score"), nr=p("non_row"), rank=p("rank"), hist=p("hist"),
               rank_hist=p("rank_hist"), counts=p("counts"))
    for kw in finish_refusals():                                               # a misaligned address: the real one plus 4
        kw = {k: (v if v is None or k in ("M", "nbins") else fin[k] + v % 8) for k, v in kw.items()}
        assert call_finish(L, **{**fin, **kw}) == -22, kw
    keys = torch.zeros(M, dtype=torch.int64, device=DEV)
    for bad in (lambda: ops.ident_best(a.cpu(), la, mate_key=keys, non_key=keys, skipped=keys[:1]),
                lambda: ops.ident_best(a, la, mate_key=keys[:50], non_key=keys, skipped=keys[:1]),
                lambda: ops.ident_best(a, la, mate_key=keys.int(), non_key=keys, skipped=keys[:1]),
                lambda: ops.ident_best(a, la, None, la, mate_key=keys, non_key=keys, skipped=keys[:1]),
                lambda: ops.ident_best(a, la, mate_key=keys, non_key=keys, skipped=keys[:1], b_row0=3),
                lambda: ops.ident_best(a, la, a, mate_key=keys, non_key=keys, skipped=keys[:1]),
                lambda: ops.ident_rank(a[:, :500], la, mate_key=keys, rank_minus_1=keys.int()),
                lambda: ops.ident_rank(a, la, mate_key=keys, rank_minus_1=keys),
                lambda: ops.ident_finish(la, mate_key=keys, non_key=keys, nbins=100, hist=out.v("hist"),
                                         counts=out.v("counts"), **{k: out.v(k) for k in PER_PROBE}),
                lambda: ops.ident_finish(la, mate_key=keys, non_key=keys, nbins=2048, hist=out.v("hist"),
                                         counts=out.v("counts"), rank_hist=out.v("rank_hist"),
                                         **{k: out.v(k) for k in PER_PROBE})):
        with pytest.raises(ValueError):
            bad()
    got = out.host()
    for k in ("mate_key", "non_key", "rank_minus_1", "hist", "rank_hist", "counts"):
        assert not got[k].any(), k
    assert got["skipped"] == 0 and int(keys.sum()) == 0
    for k in PER_PROBE:
        assert (got[k] == ISENT).all(), k


# ---------------------------------------------------------------------------------- 8. planted identities
def test_planted_identities_against_fp64():
    """40 identities x 6 rows and 60 strangers at D = 128 (tests/test_identeval_host.py asserts that
    every deciding margin is above 2 x PLANTED_TOL and 4 e_ref below PLANTED_TOL): rows, ranks,
    histograms and counts equal the fp64 statement, scores lie within PLANTED_TOL."""
    ref = planted_reference()
    rows, labels, q = enrol(ref["x"]), ref["labels"], torch.from_numpy(ref["in_gallery"]).to(DEV)
    cases = (("cross", run(rows[~q].contiguous(), labels[ref["in_gallery"] == 0], rows[q].contiguous(),
                           labels[ref["in_gallery"]], nbins=ref["nbins"])),
             ("self", run(rows, labels, nbins=ref["nbins"])))
    for name, got in cases:
        want = ref[name]
        for k in ("mate_row", "non_row", "rank", "hist", "rank_hist", "counts"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} {k}")
        for k in ("mate_score", "non_score"):
            there = np.isfinite(want[k])
            err = np.abs(got[k][there].astype(np.float64) - want[k][there]).max()
            print(f"ident planted {name} {k}: max |gpu - fp64| = {err:.3e}, e_ref = {ref['e_ref']:.3e}")
            assert err < PLANTED_TOL and np.array_equal(np.isfinite(got[k]), np.isfinite(want[k]))
        assert got["skipped"] == 0


# ---------------------------------------------------------------------------------- 9. the tile walk
@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_every_workgroup_walks_three_tiles_cross():
    tm, tn, M, N = walk_sizes_cross(cus())
    assert tiles_of(M, N) >= 3 * cus()
    a, b, la, lb, va, vb = walk_case(M, N)
    want = ident_eval_blocks(a, b, la, lb, va, vb, 256)
    same_outputs(run(a, la, b, lb, va, vb), want)
    assert want["counts"][:3].min() > 0 and (want["rank"] > 1).any() and (want["rank"] == 1).any()


def test_every_workgroup_walks_three_tiles_self():
    tn, n = walk_sizes(cus())
    assert tiles_of(n) >= 3 * cus()
    a, _, la, _, va, _ = walk_case(n, 0)
    want = ident_eval_blocks(a, None, la, None, va, None, 256)
    same_outputs(run(a, la, va=va), want)
    assert want["counts"][0] > 0 and want["counts"][2] > 0 and (want["rank"] > 1).any()


# ---------------------------------------------------------------------------------- 10. the public interface
def test_identification_eval_and_calibrate_fpir_end_to_end():
    D = 512
    g = torch.Generator().manual_seed(17)
    ids = torch.arange(30).repeat_interleave(4)
    x = (torch.randn(30, D, generator=g)[ids] + 2.5 * torch.randn(120, D, generator=g)).to(DEV)
    q = (torch.arange(120) % 4 < 2).to(DEV)
    strangers = torch.randn(80, D, generator=g).to(DEV)
    gal = FaceGallery(dim=D, capacity=64, device=DEV)
    gal.add(x[q], ids[q.cpu()])
    ev = IdentificationEval(gal, capacity=256)
    assert ev.add(x[~q], ids[(~q).cpu()]) == (0, 60) and ev.add(strangers, 500 + torch.arange(80)) == (60, 140)
    out = ev.compute(nbins=1024, fpir=(0.5, 0.1, 0.0))
    assert (out["mated"], out["non_mated"], out["left_out"], out["no_candidate"], out["skipped"]) == (60, 80, 0, 0, 0)
    dev = ev.evaluate(nbins=1024)
    host = {k: (v.cpu().numpy() if v is not None else None) for k, v in dev.items()}
    assert np.array_equal(host["hist"], out["hist"]) and host["rank_hist"].sum() == 60
    same = identification_curve(host["hist"], host["rank_hist"], host["counts"], fpir=(0.5, 0.1, 0.0))
    assert same["at_fpir"] == out["at_fpir"] and np.array_equal(same["cmc"], out["cmc"])
    assert out["cmc"][0] == (host["rank"] == 1).sum() / 60 and out["cmc"][-1] <= 1.0
    # calibrate_fpir: at the row's edge the strangers identify names meet the target, one edge lower they do not
    fid = FaceIdentifier(None, gal)
    row = fid.calibrate_fpir(ev, 0.1)
    assert fid.threshold == row["threshold"] and row == ev.compute(nbins=2048, fpir=(0.1,), cmc=False)["at_fpir"][0]
    named = lambda t: int((gal.identify(strangers, t)[0] >= 0).sum())
    lower = float(thresholds_ref(2048)[row["bin"] - 1])
    assert named(fid.threshold) == row["false_positives"] <= 8 < named(lower)
    right = int((gal.identify(x[~q], fid.threshold)[0].cpu() == ids[(~q).cpu()]).sum())
    assert right == row["right_names"] and row["dir"] == right / 60
    # leave-one-out on the gallery: two rows per identity, so every row has one mate
    loo = IdentificationEval.leave_one_out(gal).compute(nbins=256)
    assert (loo["mated"], loo["non_mated"]) == (60, 0) and np.isnan(loo["curve"]["fpir"]).all()
    gal.remove([0])
    loo = IdentificationEval.leave_one_out(gal).compute(nbins=256, cmc=False)
    assert (loo["mated"], loo["non_mated"], loo["left_out"]) == (58, 0, 2) and loo["cmc"] is None
