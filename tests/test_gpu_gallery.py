"""GPU: face identification (csrc/gallery.hip) -- prpe_gallery_enrol and the fused
cosine top-k prpe_gallery_topk -- against the fp64 restatement of the stated rule
(tests/test_gallery_host.py, ``gallery_topk_ref``) on the CPU.

Outputs live in sentinel-filled buffers with guard floats on both sides (``Guarded``,
tests/test_gpu_rowops.py); every launch is followed by a check that the guards are untouched.

Scores: per case e_ref = the largest distance of the fp32 CPU evaluation (F.normalize + matmul)
from the fp64 one over the whole [Q, G] score matrix of the same inputs; the kernel's scores may
be 4 e_ref from the fp64 score of the row they name (the margin the top-down and pose-eval tests
give fp32 noise: another summation order). Rows are compared exactly for every query whose top
k + 1 fp64 scores are pairwise further apart than 2 x that bound, and the fixed seeds are such that
this is EVERY query (asserted: nothing is exempt). Shapes: every Q in {1, 17, 37, 130}, G in
{1, 5, 70, 1025, 4099}, D in {32, 96, 512} and k in {1, 5, 8} occurs, in combinations that keep
at least 70 scores per case, so that e_ref is a maximum over a sample and not one number: both
query routes (Q <= 16 and wider), Q and G off every tile / chunk multiple (the chunk is 64 rows at
these G; one tie case uses a G past 32768 where it is 128), G < k.

Measured on an MI355X (kernel max error / e_ref per case): see DESIGN.md §5d.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from prpe import CombinedModel, FaceGallery, FaceIdentifier, FrameIngest, ops
from test_gallery_host import gallery_topk_ref
from test_gpu_rowops import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
ISENT = -7777


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------- harness
class Store:
    """A guarded gallery [capacity, D] + norms [capacity] enrolled from host rows."""

    def __init__(self, x, capacity=None, splits=None):
        n, D = x.shape
        self.cap = capacity or n
        self.rows, self.norms = Guarded((self.cap, D)), Guarded((self.cap,))
        xd = x.to(DEV)
        edges = [0] + list(splits or []) + [n]
        for a, b in zip(edges[:-1], edges[1:]):
            ops.gallery_enrol(xd[a:b].contiguous(), self.rows.view, self.norms.view, a)

    def check(self):
        assert self.rows.untouched() and self.norms.untouched()


def topk(q, store, G, k, valid=None, labels=None, threshold=0.0):
    """One guarded launch -> host (scores, rows[, ident])."""
    Q = q.shape[0]
    s, r = Guarded((Q, k)), Guarded((Q, k), fill=ISENT, dtype=torch.int32)
    ident = Guarded((Q,), fill=ISENT, dtype=torch.int64) if labels is not None else None
    ops.gallery_topk(q.to(DEV), store.rows.view, G, k, scores=s.view, rows=r.view,
                     valid=None if valid is None else valid.to(DEV),
                     labels=None if labels is None else labels.to(DEV), threshold=threshold,
                     ident=None if ident is None else ident.view)
    assert s.untouched() and r.untouched() and (ident is None or ident.untouched())
    out = (s.cpu(), r.cpu())
    return out if ident is None else out + (ident.cpu(),)


def make(Q, G, D, seed):
    """Gallery rows and queries from one seeded generator; the first half of the queries are
    gallery rows plus 0.3 x noise (a real probe), the rest are unrelated."""
    g = torch.Generator().manual_seed(seed)
    gal = torch.randn(G, D, generator=g)
    q = torch.randn(Q, D, generator=g)
    for i in range((Q + 1) // 2):
        q[i] = gal[(i * 7) % G] + 0.3 * q[i]
    return q, gal


@functools.lru_cache(maxsize=None)
def case(Q, G, D, seed):
    """Inputs, the enrolled store, the fp64 score matrix and e_ref -- computed once per shape."""
    q, gal = make(Q, G, D, seed)
    s64 = F.normalize(q.double(), dim=1) @ F.normalize(gal.double(), dim=1).t()
    s32 = F.normalize(q, dim=1) @ F.normalize(gal, dim=1).t()
    e_ref = float((s32.double() - s64).abs().max())
    return q, gal, Store(gal), s64, e_ref


SEED = 7
SHAPES = [(130, 1, 512), (37, 5, 96), (130, 5, 32), (17, 70, 32), (130, 70, 96), (1, 70, 512), (1, 1025, 512),
          (17, 1025, 96), (37, 1025, 32), (130, 1025, 512), (1, 4099, 96), (1, 4099, 512), (17, 4099, 32),
          (37, 4099, 512)]
# generator seed 7 everywhere but at 37 x 4099 x 512, where it puts two queries' 8th and 9th fp64
# scores 1.3e-6 apart (closer than 2 x the bound): replaced by seed 8, not exempted
SEEDS = {shape: SEED for shape in SHAPES}
SEEDS[(37, 4099, 512)] = 8


def shape_case(Q, G, D):
    return case(Q, G, D, SEEDS[(Q, G, D)])


def exempt_queries(s64, k, bound):
    """Queries with two of their top k + 1 fp64 scores closer than 2 x bound."""
    top = torch.sort(s64, dim=1, descending=True).values[:, :k + 1]
    if top.shape[1] < 2:
        return torch.zeros(s64.shape[0], dtype=torch.bool)
    return ((top[:, :-1] - top[:, 1:]) <= 2 * bound).any(dim=1)


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("Q,G,D", SHAPES)
def test_scores_within_four_e_ref_and_rows_exact(Q, G, D, k):
    q, gal, store, s64, e_ref = shape_case(Q, G, D)
    bound = 4 * e_ref
    s, r = topk(q, store, G, k)
    store.check()
    want_s, want_r = gallery_topk_ref(q, gal, k)
    n = min(G, k)
    assert (r[:, n:] == -1).all() and torch.isneginf(s[:, n:]).all()           # G < k: the tail is (-1, -inf)
    assert ((r[:, :n] >= 0) & (r[:, :n] < G)).all()
    err = float((s[:, :n].double() - torch.gather(s64, 1, r[:, :n].long())).abs().max())
    exempt = exempt_queries(s64, k, bound)
    print(f"gallery Q={Q} G={G} D={D} k={k}: e_ref={e_ref:.3e} kernel={err:.3e} ratio={err / max(e_ref, 1e-30):.2f} "
          f"exempt={int(exempt.sum())}")
    assert err <= bound
    assert not exempt.any()                  # the seed leaves no query to exempt
    assert torch.equal(r, want_r)
    assert (s[:, :n - 1] >= s[:, 1:n]).all()


# ---------------------------------------------------------------------------------- ties and order
def _tie_case(Q, G, D, pos, seed):
    g = torch.Generator().manual_seed(seed)
    gal = torch.randn(G, D, generator=g)
    for p in pos:
        gal[p] = gal[pos[0]]
    q = torch.randn(Q, D, generator=g)
    q[0] = gal[pos[0]] + 0.05 * q[0]
    return q, gal


G4 = 4099
TIES = [
    # the first and last row, both sides of the first 16-row tile and 64-row step / chunk boundaries
    (1, G4, 96, [0, 15, 16, 63, 64, 65, G4 - 1]),
    (17, G4, 96, [0, 15, 16, 63, 64, 65, G4 - 1]),
    (1, G4, 96, [31, 32, 47, 48, 127, 128, 4095, 4096]),
    (37, G4, 512, [31, 32, 47, 48, 127, 128, 4095, 4096]),
    # the last tiles: the final step holds 3 rows
    (1, G4, 512, [4031, 4032, 4047, 4048, 4095, 4096, 4097, 4098]),
    (130, G4, 32, [4031, 4032, 4047, 4048, 4095, 4096, 4097, 4098]),
    # 128-row chunks (G past 512 x 64): both sides of a chunk boundary, of the step boundary inside
    # a chunk, and of the last chunk's start
    (17, 32835, 32, [127, 128, 129, 191, 192, 32767, 32768, 32834]),
]


@pytest.mark.parametrize("Q,G,D,pos", TIES)
def test_exact_duplicates_tie_and_come_in_ascending_row_order(Q, G, D, pos):
    qb, nqb, chunk, nchunks = ops.gallery_plan(Q, G)
    assert chunk == (128 if G > 32768 else 64)
    q, gal = _tie_case(Q, G, D, pos, 11)
    store = Store(gal)
    s, r = topk(q, store, G, 8)
    want_s, want_r = gallery_topk_ref(q, gal, 8)
    n = min(len(pos), 8)
    assert r[0, :n].tolist() == sorted(pos)[:n]
    assert (_bits(s[0, :n]) == _bits(s[0, :1])).all()                  # the same bits wherever the row lies
    # after the duplicates, the reference's next rows (the CPU's fp64 matmul does not give the
    # duplicates the same bits at every row, so their order is taken from the rule, not from it)
    rest = [int(v) for v in want_r[0] if int(v) not in pos]
    assert r[0].tolist() == (sorted(pos) + rest)[:8]
    assert abs(float(s[0, 0]) - float(want_s[0, 0])) <= 1e-6


def test_best_match_at_the_first_and_the_last_row():
    q, gal, store, s64, e_ref = shape_case(37, 4099, 512)
    probe = torch.stack([gal[0], gal[4098], gal[0] * 3.0, -gal[4098]])
    s, r = topk(probe, store, 4099, 1)
    assert r[:3, 0].tolist() == [0, 4098, 0] and r[3, 0] != 4098
    assert (s[:3, 0] - 1).abs().max() <= 4 * e_ref


# ---------------------------------------------------------------------------------- mask, NaN, zero
def test_masked_rows_never_appear_and_few_valid_rows_pad_the_tail():
    q, gal, store, s64, e_ref = shape_case(17, 1025, 96)
    g = torch.Generator().manual_seed(3)
    valid = (torch.rand(1025, generator=g) > 0.3).to(torch.uint8)
    valid[gallery_topk_ref(q, gal, 1)[1][:, 0].long()] = 0           # every query's best row is masked
    s, r = topk(q, store, 1025, 8, valid=valid)
    want_s, want_r = gallery_topk_ref(q, gal, 8, valid=valid)
    assert valid[r.long()].all() and torch.equal(r, want_r)
    assert (s.double() - want_s).abs().max() <= 4 * e_ref
    few = torch.zeros(1025, dtype=torch.uint8)
    few[[3, 700, 1024]] = 1
    s, r = topk(q, store, 1025, 8, valid=few)
    want_s, want_r = gallery_topk_ref(q, gal, 8, valid=few)
    assert torch.equal(r, want_r) and (r[:, 3:] == -1).all() and torch.isneginf(s[:, 3:]).all()
    assert sorted(r[0, :3].tolist()) == [3, 700, 1024]
    s, r = topk(q[:1], store, 1025, 5, valid=torch.zeros(1025, dtype=torch.uint8))      # nothing valid at all
    assert (r == -1).all() and torch.isneginf(s).all()


@pytest.mark.parametrize("Q", [3, 37])
def test_nan_and_infinite_rows_are_skipped_and_a_zero_query_scores_zero(Q):
    q, gal = make(Q, 70, 96, 5)
    gal, q = gal.clone(), q.clone()
    gal[7, 5] = float("nan")
    gal[9, 0] = float("inf")
    gal[64] = float("nan")
    gal[40] = 0.0                                   # a zero row stays zero: score 0 against everything
    q[1, 17] = float("nan")
    q[2] = 0.0
    q[0] = gal[40 - 1] + 0.01 * q[0]
    store = Store(gal)
    assert torch.equal(store.rows.view[40].cpu(), torch.zeros(96))
    s, r = topk(q, store, 70, 8)
    want_s, want_r = gallery_topk_ref(q, gal, 8)
    assert torch.equal(r, want_r)
    assert not torch.isin(r, torch.tensor([7, 9, 64], dtype=torch.int32)).any()
    assert (r[1] == -1).all() and torch.isneginf(s[1]).all()                       # the NaN query matches nothing
    assert r[2].tolist() == [0, 1, 2, 3, 4, 5, 6, 8] and (s[2] == 0).all()         # rows in order, 7 is NaN
    ok = r >= 0
    assert (s.double() - want_s)[ok].abs().max() <= 1e-6


# ---------------------------------------------------------------------------------- ident
@pytest.mark.parametrize("Q", [1, 17])
def test_ident_threshold_is_inclusive_to_the_ulp_and_labels_are_int64(Q):
    q, gal, store, s64, e_ref = shape_case(17, 1025, 96)
    q = q[:Q]
    labels = torch.arange(1025, dtype=torch.int64) * (2 ** 33) + 5
    s0, r0 = topk(q, store, 1025, 1)
    top = s0[0, 0]
    for thr in (top, torch.nextafter(top, torch.tensor(2.0)), torch.nextafter(top, torch.tensor(-2.0))):
        s, r, ident = topk(q, store, 1025, 1, labels=labels, threshold=float(thr))
        assert torch.equal(_bits(s), _bits(s0)) and torch.equal(r, r0)
        want = torch.where(s[:, 0] >= thr, labels[r[:, 0].long()], torch.tensor(-1))
        assert torch.equal(ident, want)
        assert int(ident[0]) == (-1 if thr > top else int(labels[r0[0, 0]]))
    assert int(labels[r0[0, 0]]) > 2 ** 32 or int(r0[0, 0]) == 0
    s, r, ident = topk(q, store, 1025, 1, valid=torch.zeros(1025, dtype=torch.uint8), labels=labels, threshold=-2.0)
    assert (ident == -1).all()                                     # no valid row: -1 whatever the threshold


# ---------------------------------------------------------------------------------- independence
def test_enrol_in_one_call_and_in_two_gives_the_same_bytes_and_the_norms():
    q, gal = make(2, 70, 96, 9)
    one, two = Store(gal, capacity=75), Store(gal, capacity=75, splits=[37])
    one.check()
    two.check()
    assert torch.equal(_bits(one.rows.buf), _bits(two.rows.buf)) and torch.equal(_bits(one.norms.buf), _bits(two.norms.buf))
    want = F.normalize(gal.double(), dim=1)
    assert (one.rows.view[:70].cpu().double() - want).abs().max() <= 2e-7
    assert torch.allclose(one.norms.view[:70].cpu().double(), gal.double().norm(dim=1), rtol=1e-6, atol=0)


def test_a_score_does_not_depend_on_the_batch_the_route_or_the_gallery_size():
    q, gal, store, s64, e_ref = shape_case(130, 1025, 512)
    s, r = topk(q, store, 1025, 8)
    s1, r1 = topk(q[:1], store, 1025, 8)                            # the Q <= 16 route
    assert torch.equal(_bits(s1[0]), _bits(s[0])) and torch.equal(r1[0], r[0])
    s17, r17 = topk(q[40:57], store, 1025, 8)                       # other batch-mates, another tile position
    assert torch.equal(_bits(s17), _bits(s[40:57])) and torch.equal(r17, r[40:57])
    s2, r2 = topk(q, store, 1025, 8)                                # two runs: the same bits
    assert torch.equal(_bits(s2), _bits(s)) and torch.equal(r2, r)


def test_the_first_rows_of_a_larger_gallery_give_the_same_bits():
    q, gal, big, s64, e_ref = shape_case(37, 4099, 512)
    small = Store(gal[:1025])
    for qq in (q, q[:1]):
        sa, ra = topk(qq, big, 1025, 8)
        sb, rb = topk(qq, small, 1025, 8)
        assert torch.equal(_bits(sa), _bits(sb)) and torch.equal(ra, rb)


# ---------------------------------------------------------------------------------- end to end
def test_face_identifier_end_to_end_at_64x64(state_dict):
    model = CombinedModel(state_dict, device=DEV)
    model.set_task("pose_estimation")
    g = torch.Generator().manual_seed(31)
    u8 = torch.randint(0, 256, (7, 64, 64, 3), generator=g, dtype=torch.uint8)
    ing = FrameIngest(size=(64, 64), mode="stretch", norm="unit")
    x = (u8.permute(0, 3, 1, 2).float() * torch.tensor(ing.a).view(1, 3, 1, 1)
         + torch.tensor(ing.b).view(1, 3, 1, 1)).to(DEV)
    labels = [2 ** 35 + i for i in range(6)]
    fid = FaceIdentifier(model, FaceGallery(dim=512, capacity=8, device=DEV), threshold=0.0)
    assert fid.enrol(x[:6], labels) == (0, 6) and len(fid.gallery) == 6
    emb = fid.embed(x).cpu()
    s64 = F.normalize(emb.double(), dim=1) @ F.normalize(emb[:6].double(), dim=1).t()
    s32 = F.normalize(emb, dim=1) @ F.normalize(emb[:6], dim=1).t()
    bound = 4 * float((s32.double() - s64).abs().max())
    other_best = float(s64[6].max())
    off = s64[:6].clone()
    off.fill_diagonal_(-1.0)
    print(f"face e2e: bound={bound:.3e} other frame's best={other_best:.6f} enrolled frames' closest pair={float(off.max()):.6f}")
    assert other_best < 1 - 4 * bound and float(off.max()) < 1 - 4 * bound     # the synthetic faces are distinct
    fid.threshold = 0.5 * (other_best + 1.0)
    ident, score = fid(x)
    assert ident[:6].tolist() == labels and int(ident[6]) == -1
    assert (score[:6].cpu() - 1).abs().max() <= bound
    assert abs(float(score[6]) - other_best) <= bound
    ident8, score8 = fid.from_frames_u8(u8.to(DEV), ing)
    assert torch.equal(ident8, ident) and torch.equal(_bits(score8), _bits(score))
    sc, rows, lab = fid.gallery.search(fid.embed(x[:2]), k=3)
    assert rows[:, 0].tolist() == [0, 1] and lab[:, 0].tolist() == labels[:2]
    fid.gallery.remove([labels[0]])
    ident, score = fid(x[:2])
    assert int(ident[0]) != labels[0] and int(ident[1]) == labels[1]
    assert model.current_task == "pose_estimation"                  # the task state is left alone
