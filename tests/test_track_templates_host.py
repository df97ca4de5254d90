"""CPU: track-level face templates (csrc/tracktemplate.hip, prpe.tracks) as far as the host goes --
``track_template_update_ref`` / ``track_template_assign_ref``, plain loops per slot, person and
element on Python integers and ``np.float32`` written from include/prpe.h alone
(tests/test_gpu_track_templates.py holds the kernels to them by equality), a second, vectorised
statement that adds the contributions in reverse order, the scenarios both files share, the bound
arithmetic, the refusals of ``ops`` and ``PersonTracker`` and the margins of the fusion scenarios.

Tolerance: none anywhere. The sums are integers and a query row is one fixed conversion of them."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from prpe import _lib

NAN, INF = float("nan"), float("inf")
SLOTS = 32
LIMIT = 1 << 20
F32 = np.float32
SCALE = F32(2.0 ** 24)
STATE_KEYS = ("tmpl_owner", "tmpl_sum", "tmpl_n", "tmpl_ident", "tmpl_score")


def fresh_templates(S, D):
    return {"tmpl_owner": np.full((S, SLOTS), -1, np.int32), "tmpl_sum": np.zeros((S, SLOTS, D), np.int64),
            "tmpl_n": np.zeros((S, SLOTS), np.int32), "tmpl_ident": np.full((S, SLOTS), -1, np.int64),
            "tmpl_score": np.full((S, SLOTS), -np.inf, np.float32)}


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


# ---------------------------------------------------------------------------------- the restatement
def term(w, e):
    """llrintf((w * e) * 2^24): one fp32 product, an exact scaling, round half to even."""
    p = F32(w) * F32(e)
    return int(np.rint(np.float64(p * SCALE)))


def track_template_update_ref(c, state, max_q):
    """prpe_track_template_update on the host; ``c`` is a call (see ``make_call``). Returns
    (state after, dirty_rows, n_dirty, dirty_pos, queries); the state passed in is left as it is."""
    st = copy_state(state)
    S, D = st["tmpl_sum"].shape[0], st["tmpl_sum"].shape[2]
    emb, norms = c["emb"], c["norms"]
    P, Fcap, B = c["meta_p"].shape[0], emb.shape[0], len(c["frame_stream"])
    n_p, n_f = max(0, min(int(c["n_p"]), P)), max(0, min(int(c["n_f"]), Fcap))
    frame = c["meta_p"].view(np.int32)[:, 0]
    ids = c["trk_meta"].view(np.int32)[:, :, 0]
    dirty = []
    for s in range(S):
        for j in range(SLOTS):
            tid = int(ids[s, j])
            if tid < 0 or int(st["tmpl_owner"][s, j]) != tid:
                st["tmpl_sum"][s, j] = 0
                st["tmpl_n"][s, j], st["tmpl_ident"][s, j], st["tmpl_score"][s, j] = 0, -1, -np.inf
                st["tmpl_owner"][s, j] = tid if tid >= 0 else -1
            if tid < 0:
                continue
            took = 0
            for i in range(n_p):
                b = int(frame[i])
                if not 0 <= b < B or int(c["frame_stream"][b]) != s or int(c["track_id"][i]) != tid:
                    continue
                f = int(c["person_face"][i])
                if not 0 <= f < n_f:
                    continue
                nv = norms[f]
                if not (np.isfinite(nv) and nv >= F32(c["min_norm"]) and nv < F32(32768.0)):
                    continue
                if not all(np.isfinite(emb[f, d]) for d in range(D)):
                    continue
                if int(st["tmpl_n"][s, j]) >= LIMIT:
                    continue
                w = nv if c["weight_mode"] == 0 else F32(1.0)
                for d in range(D):
                    st["tmpl_sum"][s, j, d] = int(st["tmpl_sum"][s, j, d]) + term(w, emb[f, d])
                st["tmpl_n"][s, j] += 1
                took += 1
            if took:
                dirty.append(s * SLOTS + j)
    dirty_pos = np.full((S, SLOTS), -1, np.int32)
    dirty_rows = np.full(max_q, -1, np.int32)
    queries = np.zeros((max_q, D), np.float32)
    for r, g in enumerate(dirty):
        dirty_pos[g // SLOTS, g % SLOTS] = r            # at or past max_q: dirty, but in no list
        if r < max_q:
            dirty_rows[r] = g
            for d in range(D):
                queries[r, d] = F32(np.float64(int(st["tmpl_sum"][g // SLOTS, g % SLOTS, d])) * 2.0 ** -24)
    return st, dirty_rows, np.array([min(len(dirty), max_q)], np.int32), dirty_pos, queries


def track_template_assign_ref(c, state, ident, score, n_dirty, dirty_rows, dirty_pos):
    """prpe_track_template_assign on the host: (state after, template_ident, template_score,
    template_faces)."""
    st = copy_state(state)
    S = st["tmpl_n"].shape[0]
    P, B = c["meta_p"].shape[0], len(c["frame_stream"])
    n_p = max(0, min(int(c["n_p"]), P))
    nd = max(0, min(int(n_dirty[0]), len(ident)))
    for r in range(nd):
        g = int(dirty_rows[r])
        st["tmpl_ident"][g // SLOTS, g % SLOTS] = ident[r]
        st["tmpl_score"][g // SLOTS, g % SLOTS] = score[r]
    t_ident, t_score = np.full(P, -1, np.int64), np.full(P, -np.inf, np.float32)
    t_faces = np.zeros(P, np.int32)
    frame = c["meta_p"].view(np.int32)[:, 0]
    ids = c["trk_meta"].view(np.int32)[:, :, 0]
    for i in range(n_p):
        b, tid = int(frame[i]), int(c["track_id"][i])
        if tid < 0 or not 0 <= b < B:
            continue
        s = int(c["frame_stream"][b])
        if not 0 <= s < S:
            continue
        for j in range(SLOTS):
            if int(ids[s, j]) == tid:
                t_ident[i], t_score[i], t_faces[i] = st["tmpl_ident"][s, j], st["tmpl_score"][s, j], st["tmpl_n"][s, j]
                break
    return st, t_ident, t_score, t_faces


# ---------------------------------------------------------------------------------- the second statement
def update_plain(c, state, max_q):
    """include/prpe.h's template update once more: whole arrays at a time, the contributions of a
    slot added last first. Written apart from ``track_template_update_ref``."""
    own, tot, cnt = state["tmpl_owner"].copy(), state["tmpl_sum"].copy(), state["tmpl_n"].copy()
    name, sc = state["tmpl_ident"].copy(), state["tmpl_score"].copy()
    S, _, D = tot.shape
    E, nrm = np.asarray(c["emb"], np.float32), np.asarray(c["norms"], np.float32)
    P, B = len(c["track_id"]), len(c["frame_stream"])
    n_p, n_f = int(np.clip(c["n_p"], 0, P)), int(np.clip(c["n_f"], 0, E.shape[0]))
    ids = np.ascontiguousarray(c["trk_meta"][:, :, 0]).view(np.int32)
    wipe = (ids < 0) | (own != ids)
    tot[wipe], cnt[wipe], name[wipe], sc[wipe] = 0, 0, -1, -np.inf
    own = np.where(ids < 0, -1, ids).astype(np.int32)
    with np.errstate(all="ignore"):
        good = np.isfinite(nrm) & (nrm >= F32(c["min_norm"])) & (nrm < F32(2.0 ** 15)) & np.isfinite(E).all(axis=1)
        good[n_f:] = False
        w = nrm if c["weight_mode"] == 0 else np.ones_like(nrm)
        fixed = np.zeros(E.shape, np.int64)
        fixed[good] = np.rint(((w[good, None] * E[good]).astype(np.float32) * SCALE).astype(np.float64)).astype(np.int64)
    fr = np.ascontiguousarray(c["meta_p"][:n_p, 0]).view(np.int32)
    inside = (fr >= 0) & (fr < B)
    stream = np.where(inside, np.asarray(c["frame_stream"])[np.clip(fr, 0, B - 1)], -1)
    face = np.asarray(c["person_face"])[:n_p]
    tid = np.asarray(c["track_id"])[:n_p]
    usable = inside & (face >= 0) & (face < n_f) & good[np.clip(face, 0, E.shape[0] - 1)]
    flags = np.zeros((S, SLOTS), bool)
    for s, j in zip(*np.nonzero(ids >= 0)):
        rows = np.nonzero(usable & (stream == s) & (tid == ids[s, j]))[0][:max(LIMIT - int(cnt[s, j]), 0)]
        if rows.size:
            tot[s, j] += fixed[face[rows[::-1]]].sum(axis=0)
            cnt[s, j] += rows.size
            flags[s, j] = True
    order = np.cumsum(flags.reshape(-1)) - 1
    pos = np.where(flags.reshape(-1), order, -1).astype(np.int32).reshape(S, SLOTS)
    listed = np.nonzero(flags.reshape(-1))[0][:max_q]
    rows_out = np.full(max_q, -1, np.int32)
    rows_out[:listed.size] = listed
    q = np.zeros((max_q, D), np.float32)
    q[:listed.size] = (tot.reshape(-1, D)[listed].astype(np.float64) * 2.0 ** -24).astype(np.float32)
    new = {"tmpl_owner": own, "tmpl_sum": tot, "tmpl_n": cnt, "tmpl_ident": name, "tmpl_score": sc}
    return new, rows_out, np.array([listed.size], np.int32), pos, q


# ---------------------------------------------------------------------------------- calls and scenarios
def trk_meta_of(ids):
    """trk_meta [S, 32, 8] whose id column holds ``ids`` [S, 32]; the other columns hold a pattern."""
    ids = np.asarray(ids, np.int32)
    m = np.full((*ids.shape, 8), 3.25, np.float32)
    m.view(np.int32)[:, :, 0] = ids
    return m


def make_call(ids, persons, emb, norms, frame_stream, n_p=None, n_f=None, max_p=None, weight_mode=0, min_norm=0.0):
    """``persons``: (frame, track_id, face) per person slot. Slots behind n_p hold a stale row."""
    n = len(persons)
    P = max_p or n + 1
    meta = np.full((P, 8), 1.5, np.float32)
    meta.view(np.int32)[:, 0] = 0
    tid, face = np.zeros(P, np.int32), np.zeros(P, np.int32)       # a stale row: frame 0, track 0, face 0
    for i, (b, t, f) in enumerate(persons):
        meta.view(np.int32)[i, 0], tid[i], face[i] = b, t, f
    return {"meta_p": meta, "n_p": n if n_p is None else n_p, "track_id": tid, "person_face": face,
            "emb": np.asarray(emb, np.float32), "norms": np.asarray(norms, np.float32),
            "n_f": len(norms) if n_f is None else n_f, "frame_stream": np.asarray(frame_stream, np.int32),
            "trk_meta": trk_meta_of(ids), "weight_mode": weight_mode, "min_norm": min_norm}


def unit_rows(n, D, seed):
    e = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
    return (e / np.sqrt((e.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(np.float32)


def ids_with(S, live):
    """[S, 32] ids, -1 but for ``live`` = {(s, j): id}."""
    ids = np.full((S, SLOTS), -1, np.int32)
    for (s, j), v in live.items():
        ids[s, j] = v
    return ids


def _random_calls(S, D, seed):
    """Two calls of 129 persons in 130 slots over 6 frames and 64 face slots (60 filled): persons of
    live tracks, of dead tracks and of none, faces of every kind, a frame of stream -1 and one of
    stream S, frame indices outside [0, B); the second call reuses one slot, frees one and leaves
    others without a face."""
    rng = np.random.default_rng(seed)
    B, F, n_f = 6, 64, 60
    emb, norms = unit_rows(F, D, seed + 1), (rng.random(F) * 30 + 5).astype(np.float32)
    norms[7], norms[9], emb[11, D // 2] = NAN, 40000.0, INF
    fs = [b % S for b in range(B)]
    fs[4], fs[5] = -1, S
    calls = []
    live = {(s, j): 10 * s + k for s in range(S) for k, j in enumerate((0, 5, 17, 31))}
    for step in range(2):
        if step == 1:
            live[(0, 5)] = 77                                        # slot reused by another track
            del live[(S - 1, 17)]                                    # track freed
        persons = []
        for i in range(129):
            b = int(rng.integers(-1, B + 1))
            s = fs[b] if 0 <= b < B else 0
            pool = [v for (ss, _), v in live.items() if ss == s] + [-1, 500]
            face = int(rng.integers(-1, n_f + 3)) if step == 0 or i % 3 else -1
            persons.append((b, int(pool[rng.integers(len(pool))]), face))
        calls.append(make_call(ids_with(S, live), persons, emb, norms, fs, n_f=n_f, max_p=130))
    return calls


def _skip_calls(D, min_norm=2.0):
    """Every skip rule on a track of its own (slot j = case), each beside a face that does
    contribute (slot 31); one face of each kind."""
    below = float(np.nextafter(F32(min_norm), F32(-INF)))
    under = float(np.nextafter(F32(32768.0), F32(0)))
    cases = [("good", 5.0, None), ("norm_nan", NAN, None), ("norm_inf", INF, None), ("norm_below", below, None),
             ("norm_equal", min_norm, None), ("norm_2p15", 32768.0, None), ("norm_under_2p15", under, None),
             ("nan_first", 5.0, 0), ("nan_last", 5.0, D - 1), ("neg_inf_mid", 5.0, D // 2)]
    emb = unit_rows(len(cases) + 1, D, 5)
    norms = np.array([c[1] for c in cases] + [6.0], np.float32)
    for f, (_, _, at) in enumerate(cases):
        if at is not None:
            emb[f, at] = -INF if at == D // 2 else NAN
    persons = [(0, 100 + f, f) for f in range(len(cases))] + [(0, 131, len(cases))]
    live = {(0, f): 100 + f for f in range(len(cases))}
    live[(0, 31)] = 131
    return [make_call(ids_with(1, live), persons, emb, norms, [0], min_norm=min_norm)], [c[0] for c in cases]


@functools.lru_cache(maxsize=None)
def scenarios():
    """name -> (S, D, max_q, state before the first call, [calls]); the calls run one after the
    other on one state."""
    sc = {}
    for D in (32, 512):
        for S in (1, 3):
            sc[f"random_D{D}_S{S}"] = (S, D, min(S * SLOTS, 64), fresh_templates(S, D), _random_calls(S, D, 10 * S + D))
        sc[f"skips_D{D}"] = (1, D, 11, fresh_templates(1, D), _skip_calls(D)[0])
    # empty state, nobody; then a person without a face, one whose face is past n_f, one without a track
    e, n = unit_rows(4, 32, 3), [7.0, 8.0, 9.0, 10.0]
    live = ids_with(1, {(0, 2): 4, (0, 3): 6})
    sc["empty"] = (1, 32, 4, fresh_templates(1, 32),
                   [make_call(ids_with(1, {}), [], e, n, [0], max_p=130),
                    make_call(live, [(0, 4, -1), (0, 4, 3), (0, -1, 0), (0, 6, 1)], e, n, [0], n_f=3),
                    make_call(live, [(0, 6, 2), (0, 4, 0)], e, n, [0], n_p=0, max_p=3)])
    # the face limit: 2^20 - 1 faces summed already; one more is taken, the next is refused. The
    # sentinel sums of slot 0 stay (its track has no face in the call); slot 9 is cleared (reused).
    st = fresh_templates(1, 32)
    st["tmpl_owner"][0, [0, 1, 9]] = [3, 5, 8]
    st["tmpl_n"][0, [0, 1, 9]] = [12, LIMIT - 1, 40]
    st["tmpl_sum"][0, [0, 1, 9]] = np.array([777, -(1 << 58), 555])[:, None]
    st["tmpl_ident"][0, [0, 1, 9]], st["tmpl_score"][0, [0, 1, 9]] = [42, 43, 44], [0.5, 0.25, 0.75]
    sc["face_limit"] = (1, 32, 4, st, [make_call(ids_with(1, {(0, 0): 3, (0, 1): 5, (0, 9): 9}),
                                                  [(0, 5, 0), (0, 5, 1), (0, 5, 2), (0, 9, 3)], e, n, [0])])
    # uniform weights: a face that six persons of one track name is summed six times
    sc["uniform"] = (1, 32, 4, fresh_templates(1, 32),
                     [make_call(ids_with(1, {(0, 6): 2}), [(0, 2, 1)] * 6, e, n, [0], weight_mode=1)])
    # more dirty slots than the list holds (two tracks name one face slot; max_q = max_f = 2)
    sc["list_full"] = (3, 32, 2, fresh_templates(3, 32),
                       [make_call(ids_with(3, {(0, 1): 0, (1, 2): 0, (2, 30): 0, (2, 31): 1}),
                                  [(0, 0, 0), (1, 0, 1), (2, 0, 1), (2, 1, 0)], e[:2], n[:2], [0, 1, 2])])
    # five frames of two tracks in one stream, for "one call equals a call per frame"
    e5, n5 = unit_rows(10, 512, 9), np.linspace(4.0, 30.0, 10).astype(np.float32)
    sc["five_frames"] = (2, 512, 10, fresh_templates(2, 512),
                         [make_call(ids_with(2, {(0, 3): 0, (0, 4): 1, (1, 0): 0}),
                                    [(b, t, 2 * b + t) for b in range(5) for t in (0, 1)], e5, n5, [0, 0, 1, 0, 0])])
    sc["long_walk"] = (2, 32, 64, *_long_walk())
    return sc


LONG_WALK = {"a": (3, 70, 200, 255, 512, 600, 649), "b": (256, 300, 511, 513), "c": (10, 130, 515, 520, 530, 540, 640)}


def _long_walk():
    """650 persons in 700 slots: the kernel's person walk takes 256 slots per trip, so three trips,
    the last one partial. Stream 0: track 0 (slot 0) has candidates in trips 0 and 2 and none in
    trip 1, at the first and last lane of a trip among others; track 1 (slot 1) has none in trip 0,
    then some in trips 1 and 2; track 2 (slot 2) starts at 2^20 - 3 faces, takes two in trip 0, and
    in trip 2 skips a NaN norm, takes one more and refuses three. Stream 1: track 0 (slot 5) takes
    every third person of all three trips. Everybody else belongs to a dead track. The second
    call sees the first 300 slots only (two trips)."""
    rng = np.random.default_rng(77)
    emb, norms = unit_rows(64, 32, 78), (rng.random(64) * 30 + 5).astype(np.float32)
    norms[7] = NAN
    persons = [((1 if i % 2 else 3), 0, i % 64) if i % 3 == 1 else (0, 500, i % 64) for i in range(650)]
    for key, tid in (("a", 0), ("b", 1), ("c", 2)):
        for i in LONG_WALK[key]:
            persons[i] = (2 * (i % 2), tid, 7 if i == 515 else (5 * i) % 64 if (5 * i) % 64 != 7 else 8)
    ids = ids_with(2, {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 5): 0})
    st = fresh_templates(2, 32)
    st["tmpl_owner"][0, 2], st["tmpl_n"][0, 2], st["tmpl_sum"][0, 2] = 2, LIMIT - 3, 12345
    st["tmpl_ident"][0, 2], st["tmpl_score"][0, 2] = 42, 0.5
    calls = [make_call(ids, persons, emb, norms, [0, 1, 0, 1], max_p=700),
             make_call(ids, persons, emb, norms, [0, 1, 0, 1], n_p=300, max_p=700)]
    return st, calls


def run(update, name):
    """[(state after, dirty_rows, n_dirty, dirty_pos, queries)] per call of the scenario."""
    S, D, max_q, state, calls = scenarios()[name]
    got = []
    for c in calls:
        got.append(update(c, state, max_q))
        state = got[-1][0]
    return got


@functools.lru_cache(maxsize=None)
def expected(name):
    return run(track_template_update_ref, name)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_arrays(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same(a, b):
    """Two results of one update call: every state array and every output, bit for bit."""
    return all(same_arrays(a[0][k], b[0][k]) for k in STATE_KEYS) and all(same_arrays(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("name", sorted(scenarios()))
def test_the_two_statements_agree(name):
    for want, got in zip(expected(name), run(update_plain, name)):
        assert same(want, got)


def test_scenarios_do_what_their_comments_say():
    _, names = _skip_calls(32)
    st, rows, nd, pos, q = expected("skips_D32")[0]
    took = {n: int(st["tmpl_n"][0, f]) for f, n in enumerate(names)}
    assert took == {"good": 1, "norm_nan": 0, "norm_inf": 0, "norm_below": 0, "norm_equal": 1, "norm_2p15": 0,
                    "norm_under_2p15": 1, "nan_first": 0, "nan_last": 0, "neg_inf_mid": 0}
    assert int(st["tmpl_n"][0, 31]) == 1 and rows[:int(nd[0])].tolist() == [0, 4, 6, 31] and int(pos[0, 31]) == 3
    assert not q[4:].any() and q[:4].any(axis=1).all()
    e = expected("empty")
    assert int(e[0][2][0]) == 0 and all(same_arrays(e[0][0][k], fresh_templates(1, 32)[k]) for k in STATE_KEYS)
    assert e[1][0]["tmpl_n"][0, :4].tolist() == [0, 0, 0, 1] and e[1][1].tolist() == [3, -1, -1, -1]
    assert e[1][0]["tmpl_owner"][0, :4].tolist() == [-1, -1, 4, 6] and same(e[2], (e[1][0], *e[0][1:]))
    st, rows, nd, pos, q = expected("face_limit")[0]
    assert st["tmpl_n"][0, [0, 1, 9]].tolist() == [12, LIMIT, 1] and st["tmpl_owner"][0, 9] == 9
    assert (st["tmpl_sum"][0, 0] == 777).all() and (st["tmpl_ident"][0, [0, 1, 9]].tolist() == [42, 43, -1])
    emb, norms = scenarios()["face_limit"][4][0]["emb"], scenarios()["face_limit"][4][0]["norms"]
    assert st["tmpl_sum"][0, 1].tolist() == [-(1 << 58) + term(norms[0], v) for v in emb[0]]
    assert rows.tolist() == [1, 9, -1, -1]
    st = expected("uniform")[0][0]
    one = [term(1.0, v) for v in scenarios()["uniform"][4][0]["emb"][1]]
    assert st["tmpl_sum"][0, 6].tolist() == [6 * v for v in one] and int(st["tmpl_n"][0, 6]) == 6
    assert one == [int(np.rint(np.float64(v) * 2.0 ** 24)) for v in scenarios()["uniform"][4][0]["emb"][1]]
    st, rows, nd, pos, q = expected("list_full")[0]
    assert int(nd[0]) == 2 and rows.tolist() == [1, 34] and pos.reshape(-1)[[1, 34, 94, 95]].tolist() == [0, 1, 2, 3]
    lw = expected("long_walk")
    call = scenarios()["long_walk"][4][0]
    third = sum(1 for i in range(650) if i % 3 == 1 and i % 64 != 7 and not any(i in v for v in LONG_WALK.values()))   # face 7: NaN norm
    assert lw[0][0]["tmpl_n"][0, :3].tolist() == [7, 4, LIMIT] and int(lw[0][0]["tmpl_n"][1, 5]) == third > 200
    taken = [call["person_face"][i] for i in (10, 130, 520)]         # 515 has a NaN norm; 530, 540 and 640 are refused
    assert lw[0][0]["tmpl_sum"][0, 2].tolist() == [12345 + sum(term(call["norms"][f], call["emb"][f, d]) for f in taken)
                                                    for d in range(32)]
    assert lw[0][1][:5].tolist() == [0, 1, 2, 37, -1] and lw[0][0]["tmpl_ident"][0, 2] == 42
    assert lw[1][0]["tmpl_n"][0, :3].tolist() == [11, 5, LIMIT] and lw[1][1][:4].tolist() == [0, 1, 37, -1]
    r = expected("random_D32_S3")
    assert int(r[0][2][0]) >= 6 and int(r[1][2][0]) >= 6
    assert int(r[1][0]["tmpl_owner"][0, 5]) == 77 and int(r[1][0]["tmpl_owner"][2, 17]) == -1
    assert not r[1][0]["tmpl_sum"][2, 17].any() and r[0][0]["tmpl_sum"][2, 17].any()


def test_bound_arithmetic():
    """|w| < 2^15 and |e| <= 1 give |w e 2^24| < 2^39; 2^20 such terms stay below 2^59 < 2^63."""
    w = np.nextafter(F32(32768.0), F32(0))
    assert abs(term(w, 1.0)) < 1 << 39 and abs(term(w, -1.0)) < 1 << 39
    assert (1 << 39) * (1 << 20) == 1 << 59 and (1 << 59) < (1 << 63) - 1
    assert LIMIT * term(w, 1.0) < (1 << 63) - 1
    assert term(1.0, 0.5) == 1 << 23 and term(2.0, F32(2.0 ** -25)) == 1       # the scaling is exact
    assert term(1.0, F32(1.5 * 2.0 ** -24)) == 2 and term(1.0, F32(2.5 * 2.0 ** -24)) == 2       # half to even


def test_assign_restatement_by_hand():
    c = make_call(ids_with(2, {(0, 3): 5, (1, 3): 5, (1, 4): 9}), [(0, 5, 0), (1, 5, 0), (1, 9, 0), (1, 8, 0), (2, 5, 0), (3, 5, 0)],
                  unit_rows(1, 32, 1), [5.0], [0, 1, 2], max_p=8)
    st = fresh_templates(2, 32)
    st["tmpl_n"][0, 3], st["tmpl_n"][1, 3], st["tmpl_n"][1, 4] = 4, 2, 7
    st["tmpl_ident"][1, 4], st["tmpl_score"][1, 4] = 21, 0.625
    pos = np.full((2, SLOTS), -1, np.int32)
    pos[0, 3], pos[1, 3] = 0, 1
    out, ti, ts, tf = track_template_assign_ref(c, st, np.array([11, 12, 99]), np.array([0.5, 0.25, 0.9], np.float32),
                                                np.array([2], np.int32), np.array([3, 35, 36], np.int32), pos)
    assert ti.tolist() == [11, 12, 21, -1, -1, -1, -1, -1] and tf.tolist() == [4, 2, 7, 0, 0, 0, 0, 0]
    assert ts.tolist() == [0.5, 0.25, 0.625] + [-INF] * 5
    assert out["tmpl_ident"][0, 3] == 11 and out["tmpl_ident"][1, 3] == 12 and out["tmpl_ident"][1, 4] == 21


# ---------------------------------------------------------------------------------- fusion: the margins
THRESHOLD = 0.5
FP32_SLACK = 1e-3       # far above what fp32 does to a cosine of D = 32 unit rows: (D + 8) * 2^-23 < 5e-6


def fusion_faces(D=32, single=0.45):
    """A gallery row g and four unit faces l2norm(g +- a n1), l2norm(g +- a n2), g, n1, n2 mutually
    orthogonal: every single cosine is 1 / sqrt(1 + a^2) = ``single``, the sum is parallel to g."""
    g, n1, n2 = (np.eye(D, dtype=np.float64)[k] for k in (0, 1, 2))
    a = math.sqrt(1.0 / single ** 2 - 1.0)
    rows = np.stack([g + a * n1, g - a * n1, g + a * n2, g - a * n2])
    rows /= np.sqrt((rows ** 2).sum(axis=1, keepdims=True))
    gallery = np.stack([g, np.eye(D)[5]])                          # labels 7 and 9
    return gallery.astype(np.float32), rows.astype(np.float32), np.full(4, 20.0, np.float32)


def outlier_faces(D=32):
    """Eight faces of the person of gallery row 0 (cosine about 0.9) and one face that is gallery
    row 1 itself: the best single frame names the track after row 1."""
    gallery = np.eye(D, dtype=np.float64)[[0, 5]]
    rng = np.random.default_rng(8)
    rows = []
    for _ in range(8):
        noise = rng.standard_normal(D)
        noise[[0, 5]] = 0.0
        noise *= math.sqrt(1.0 / 0.81 - 1.0) / np.sqrt((noise ** 2).sum())
        rows.append(gallery[0] + noise)
    rows.insert(3, gallery[1].copy())
    rows = np.stack(rows)
    rows /= np.sqrt((rows ** 2).sum(axis=1, keepdims=True))
    return gallery.astype(np.float32), rows.astype(np.float32), np.full(9, 20.0, np.float32)


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(a @ b / math.sqrt((a @ a) * (b @ b)))


def test_margins_of_the_fusion_scenarios():
    gallery, faces, norms = fusion_faces()
    single = [max(_cos(f, g) for g in gallery) for f in faces]
    fused = (norms[:, None].astype(np.float64) * faces).sum(axis=0)
    assert max(single) < THRESHOLD - 0.04 - FP32_SLACK                 # no frame names the track
    assert _cos(fused, gallery[0]) > THRESHOLD + 0.4 + FP32_SLACK      # the template does
    assert _cos(fused, gallery[0]) > _cos(fused, gallery[1]) + 0.9
    gallery, faces, norms = outlier_faces()
    right = [_cos(f, gallery[0]) for f in faces]
    wrong = [_cos(f, gallery[1]) for f in faces]
    assert wrong[3] > max(right) + 0.05 + FP32_SLACK and wrong[3] > THRESHOLD + 0.4      # the outlier wins the frames
    assert all(r > THRESHOLD + 0.3 for k, r in enumerate(right) if k != 3)
    fused = (norms[:, None].astype(np.float64) * faces).sum(axis=0)
    assert _cos(fused, gallery[0]) > _cos(fused, gallery[1]) + 0.5 + FP32_SLACK          # and loses the template
    assert _cos(fused, gallery[0]) > THRESHOLD + 0.3


# ---------------------------------------------------------------------------------- ABI, ops, PersonTracker
def test_abi_table_has_the_template_entry_points_and_the_abi_is_still_12():
    header = open(os.path.join(ROOT, "include", "prpe.h")).read()
    assert _lib.ABI_VERSION == 12 and _lib.lib().prpe_abi_version() == 12
    for name, n_args in (("prpe_track_template_update", 28), ("prpe_track_template_assign", 21)):
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/prpe.h"
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.lib(), name)


def lib_update(ptrs, max_p=4, lde=32, max_f=4, D=32, B=2, S=1, weight_mode=0, min_norm=0.0, max_q=4, null=None):
    """prpe_track_template_update on 18 device pointers in header order; ``null``: the one passed as NULL."""
    p = [None if i == null else v for i, v in enumerate(ptrs)]
    return _lib.lib().prpe_track_template_update(p[0], p[1], max_p, p[2], p[3], p[4], lde, p[5], p[6], max_f, D, p[7], B, S,
                                                 p[8], weight_mode, min_norm, *p[9:18], max_q, None)


def lib_assign(ptrs, max_p=4, B=2, S=1, max_q=4, null=None):
    """prpe_track_template_assign on 16 device pointers in header order."""
    p = [None if i == null else v for i, v in enumerate(ptrs)]
    return _lib.lib().prpe_track_template_assign(p[0], p[1], max_p, p[2], p[3], B, S, p[4], *p[5:10], max_q, *p[10:16], None)


def update_refusals():
    bad = {f"null_{i}": {"null": i} for i in range(18)}
    bad.update(B0=dict(B=0), S0=dict(S=0), S_big=dict(S=4097), P0=dict(max_p=0), F0=dict(max_f=0), D0=dict(D=0), D16=dict(D=16), D48=dict(D=48),
               D544=dict(D=544, lde=544), stride=dict(lde=31), q_small=dict(max_q=3), q_small_S=dict(max_f=40, max_q=31),
               mode2=dict(weight_mode=2), mode_neg=dict(weight_mode=-1), min_norm_nan=dict(min_norm=NAN))
    return bad


def assign_refusals():
    bad = {f"null_{i}": {"null": i} for i in range(16)}
    bad.update(B0=dict(B=0), S0=dict(S=0), S_big=dict(S=4097), P0=dict(max_p=0), Q0=dict(max_q=0))
    return bad


@pytest.mark.parametrize("name", sorted(update_refusals()))
def test_library_rejects_bad_update_arguments_before_launch(name):
    assert lib_update([0x1000] * 18, **update_refusals()[name]) == -22


@pytest.mark.parametrize("name", sorted(assign_refusals()))
def test_library_rejects_bad_assign_arguments_before_launch(name):
    assert lib_assign([0x1000] * 16, **assign_refusals()[name]) == -22


def test_ops_validate_arguments_before_any_launch():
    from prpe import ops
    assert ops.TEMPLATE_WEIGHTS == {"norm": 0, "uniform": 1} and ops.TEMPLATE_MAX_FACES == LIMIT
    meta, n = torch.zeros(4, 8), torch.zeros(1, dtype=torch.int32)
    fs, trk = torch.zeros(2, dtype=torch.int32), torch.zeros(1, 32, 8)
    rest = dict(tmpl_owner=None, tmpl_sum=None, tmpl_n=None, tmpl_ident=None, tmpl_score=None, dirty_rows=None,
                n_dirty=None, dirty_pos=None, queries=None)
    args = (meta, n, None, None, torch.zeros(4, 32), None, n, fs, trk)

    def update(i=None, v=None, **kw):
        a = list(args)
        if i is not None:
            a[i] = v
        return ops.track_template_update(*a, **{**rest, **kw})
    with pytest.raises(ValueError, match="crop_meta_p"):
        update(0, torch.zeros(8))
    with pytest.raises(ValueError, match="frame_stream"):
        update(7, [0, 0])
    with pytest.raises(ValueError, match="trk_meta"):
        update(8, torch.zeros(32, 8))
    with pytest.raises(ValueError, match="crop_meta_p"):
        update()                                                  # host tensors
    with pytest.raises(ValueError, match="crop_meta_p"):
        update(0, torch.zeros(4, 8, dtype=torch.float64))
    a_rest = dict(tmpl_n=None, tmpl_ident=None, tmpl_score=None, template_ident=None, template_score=None,
                  template_faces=None)
    with pytest.raises(ValueError, match="trk_meta"):
        ops.track_template_assign(meta, n, None, fs, torch.zeros(32, 8), None, None, n, None, None, **a_rest)
    with pytest.raises(ValueError, match="crop_meta_p"):
        ops.track_template_assign(meta, n, None, fs, trk, None, None, n, None, None, **a_rest)
    if torch.cuda.is_available():                                 # what is tested after the device checks
        dev = "cuda:0"
        d = [t.to(dev) if isinstance(t, torch.Tensor) else t for t in args]
        d[2] = d[3] = torch.zeros(4, dtype=torch.int32, device=dev)
        d[5] = torch.zeros(4, device=dev)
        for kw, what in ((dict(weight="mean"), "weight"), (dict(min_norm=NAN), "min_norm")):
            with pytest.raises(ValueError, match=what):
                ops.track_template_update(*d, **{**rest, **kw})
        d[4] = torch.zeros(4, 48, device=dev)
        with pytest.raises(ValueError, match="multiple of 32"):
            ops.track_template_update(*d, **rest)
        d[4] = torch.zeros(32, 4, device=dev).t()
        with pytest.raises(ValueError, match="embeddings"):
            ops.track_template_update(*d, **rest)


def test_tracker_constructor_and_template_state():
    from prpe import FaceGallery, PersonRecognition, PersonTracker
    pr = PersonRecognition(object(), FaceGallery(dim=512, capacity=2, device="cpu"))
    t = PersonTracker(pr)
    assert t.templates is None and t.min_norm == 0.0 and t.template_state is None
    t = PersonTracker(pr, n_streams=3, templates="uniform", min_norm=12.5)
    assert (t.templates, t.min_norm) == ("uniform", 12.5) and PersonTracker(pr, templates="norm").templates == "norm"
    for bad in (dict(templates="mean"), dict(templates=0), dict(templates="norm", min_norm=NAN), dict(min_norm=NAN)):
        with pytest.raises(ValueError, match="PersonTracker"):
            PersonTracker(pr, **bad)
    # the fresh template state is include/prpe.h's, and reset(streams) refills those streams alone
    t._state(torch.device("cpu"))
    ts = t._template_state(torch.device("cpu"), 64)
    want = fresh_templates(3, 64)
    assert set(ts) == set(STATE_KEYS) and all(same_arrays(ts[k].numpy(), want[k]) for k in STATE_KEYS)
    for v in ts.values():
        v.view(torch.int32 if v.dtype != torch.int64 else torch.int64).fill_(5)
    t.reset([0, 2])
    for k in STATE_KEYS:
        assert same_arrays(ts[k][[0, 2]].numpy(), want[k][[0, 2]]), k
        assert bool((torch.from_numpy(bits(ts[k][1].numpy())) == 5).all()), k
    with pytest.raises(ValueError, match="64-d"):             # another width would forget the templates but keep the tracks
        t._template_state(torch.device("cpu"), 32)
    assert t._template_state(torch.device("cpu"), 64) is ts
    assert t.templates_host() == [[], [], []]
    with pytest.raises(ValueError, match="enrol_track"):
        t.enrol_track(0, 3, 1)
    with pytest.raises(ValueError, match="enrol_track"):
        PersonTracker(pr).enrol_track(0, 0, 1)


def test_tracker_results_carry_the_template_fields():
    import test_tracks_host as TH
    from prpe import PersonTracker
    big = (1 << 40) + 9
    # the output test_tracks_host formats, with and without the three template arrays
    import test_faces_host as FH
    T = TH.T
    out_f = FH._face_out([[((10, 20, 30, 40), 0.9, big, 0.75)], [], [((50, 50, 70, 70), 0.7, 3, 0.5)]], 5)
    d, c = T._dets([[(10, 20, 50, 120, 0.9)], [], [(0, 0, 120, 40, 0.8), (8, 16, 200, 272, 0.7)]])
    meta, n, st = T.select_ref(d, c, max_crops=4)
    out = {"pose": {"dets": d, "counts": c, "crop_meta": meta, "n_crops": torch.tensor([n], dtype=torch.int32),
                    "status": torch.tensor([st], dtype=torch.int32), "keypoints": torch.zeros(4, 17, 3)},
           "faces": out_f, "person_face": torch.tensor([0, -1, 1, -1], dtype=torch.int32),
           "person_ident": torch.tensor([big, -1, 3, -1]), "person_score": torch.tensor([0.75, -INF, 0.5, -INF]),
           "match_status": torch.zeros(3, dtype=torch.int32), "track_id": torch.tensor([4, 0, -1, -1], dtype=torch.int32),
           "track_hits": torch.tensor([9, 1, 0, 0], dtype=torch.int32), "track_ident": torch.tensor([big, -1, -1, -1]),
           "track_ident_score": torch.tensor([0.8, -INF, -INF, -INF]), "track_status": torch.zeros(3, dtype=torch.int32)}
    plain = PersonTracker.results(out)
    assert all("template_ident" not in q for fr in plain for q in fr)
    fused = PersonTracker.results({**out, "template_ident": torch.tensor([big + 1, 6, -1, -1]),
                                   "template_score": torch.tensor([0.875, 0.25, -INF, -INF]),
                                   "template_faces": torch.tensor([31, 2, 0, 0], dtype=torch.int32)})
    assert [len(p) for p in fused] == [1, 0, 2]
    a, b, c2 = fused[0][0], fused[2][0], fused[2][1]
    assert (a["template_ident"], a["template_score"], a["template_faces"], a["track_ident"]) == (big + 1, 0.875, 31, big)
    assert (b["template_ident"], b["template_score"], b["template_faces"]) == (6, 0.25, 2)
    assert (c2["template_ident"], c2["template_score"], c2["template_faces"]) == (-1, -INF, 0)
    for p, q in zip((x for fr in plain for x in fr), (x for fr in fused for x in fr)):
        assert all(torch.equal(p[k], q[k]) if isinstance(p[k], torch.Tensor) else p[k] == q[k] for k in p)
