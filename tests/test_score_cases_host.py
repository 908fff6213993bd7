"""CPU side of tests/score_cases.py: cc_group_rectangles_levels (the host grouping with rejectLevels / levelWeights) against
the oracle's restatement over the eps and threshold grid, the Python argument rules, and checks that the shared inputs reach
the cases the GPU tests rely on them for. All comparisons are exact, weights included."""
import ctypes as C

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from oracle import oracle as orc
from tests import group_cases as gc
from tests import score_cases as sc


def _same(got, want, what):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (what, g[:8], w[:8])


def test_host_grouping_with_scores_matches_the_oracle_over_the_grid():
    lists = sc.scored_lists()
    assert len(lists) == gc.N_LISTS + 2
    for k, (r, l, w) in enumerate(lists):
        for eps in gc.EPS_GRID:
            for thr in gc.THRESHOLDS + (0,):
                m, *want = sc.oracle_group(r, l, w, thr, eps)
                got = cc.group_rectangles(r, thr, eps, levels=l, weights=w)
                assert len(got[0]) == m
                _same(got, want, (k, eps, thr))
                plain = cc.group_rectangles(r, thr, eps)
                assert plain.shape == got[0].shape and (plain == got[0]).all()  # the rectangles of the unscored call


def test_threshold_zero_copies_all_three_through():
    r, l, w = sc.scored_lists()[7]
    assert len(r) > 3
    _same(cc.group_rectangles(r, 0, levels=l, weights=w), (r, l, w), "copy")


def test_hand_made_lists():
    for (r, l, w), (want_l, want_w) in zip(sc.hand_made_lists(), sc.HAND_MADE_WANT):
        _, gl, gw = cc.group_rectangles(r, 1, levels=l, weights=w)
        assert gl.tolist() == want_l and gw.tolist() == want_w
    (_, l, w), (_, l2, w2) = sc.hand_made_lists()
    assert (l[:4] <= 0).all() and (w2[l2 == 3] < 0).all() and sc.HAND_MADE_WANT[1][0][0] == 3


def test_cap_one_short():
    r, l, w = max(sc.scored_lists(), key=lambda t: len(cc.group_rectangles(t[0], 1)))
    m, *want = sc.oracle_group(r, l, w, 1)
    assert m >= 3
    out, ol, ow = np.full((m, 4), -7, np.int32), np.full(m, -7, np.int32), np.full(m, -7.0)
    n = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = L.lib().cc_group_rectangles_levels(p(r), p(l), p(w), len(r), 1, 0.2, p(out), p(ol), p(ow), m - 1, C.byref(n))
    assert st == L.CC_ERR_BUFFER_TOO_SMALL and n.value == m
    _same((out[:m - 1], ol[:m - 1], ow[:m - 1]), [a[:m - 1] for a in want], "short")
    assert (out[m - 1] == -7).all() and ol[m - 1] == -7 and ow[m - 1] == -7.0
    m2, *short = sc.oracle_group(r, l, w, 1, cap=m - 1)  # the oracle with the same short buffer
    assert m2 == m
    _same((out[:m - 1], ol[:m - 1], ow[:m - 1]), short, "short oracle")
    st = L.lib().cc_group_rectangles_levels(p(r), None, p(w), len(r), 1, 0.2, p(out), p(ol), p(ow), m, C.byref(n))
    assert st == L.CC_ERR_INVALID_ARG


def test_python_argument_rules():
    r, l, w = sc.scored_lists()[3]
    with pytest.raises(ValueError):
        cc.group_rectangles(r, 1, levels=l)
    with pytest.raises(ValueError):
        cc.group_rectangles(r, 1, weights=w)
    with pytest.raises(ValueError):
        cc.group_rectangles(r, 1, levels=l[:-1], weights=w[:-1])
    with pytest.raises(ValueError):  # raised before any pointer is looked at, and before a device is
        cc.group_rectangles_device(0, 0, 0, 1, 0, 0, 0, levels_ptr=8, weights_ptr=8, out_levels_ptr=8)
    c = cc.CascadeClassifier()
    with pytest.raises(ValueError):
        c.detect_batch_to_device(np.zeros((1, 8, 8), np.uint8), out_ptr=0, cap=0, offsets_ptr=0, levels_ptr=8)
    with pytest.raises(ValueError):
        c.detect_batch_to_device(np.zeros((1, 8, 8), np.uint8), out_ptr=0, cap=0, offsets_ptr=0, weights_ptr=8)


def test_random_scores_hold_what_they_aim_at():
    """Every level, both signs, subnormals, DBL_MIN and repeats among the weights; classes that end at level 0 with DBL_MIN
    (no member above it) and with a member's weight; classes of level >= 1 whose best weight is negative; classes whose best
    weight is neither the first nor the last member's."""
    lists = sc.scored_lists()[:gc.N_LISTS]
    allw = np.concatenate([w for _, _, w in lists])
    alll = np.concatenate([l for _, l, _ in lists])
    assert set(alll.tolist()) == set(sc.LEVELS)
    assert (allw == sc.DBL_MIN).any() and ((np.abs(allw) < sc.DBL_MIN) & (allw != 0)).any() and (allw < 0).any() and (allw > 1).any()
    assert not np.isnan(allw).any() and not (np.signbit(allw) & (allw == 0)).any()
    assert sum(len(np.unique(w)) < len(w) for _, _, w in lists if len(w) > 1) > 50
    zero_min = zero_member = neg_best = 0
    for r, l, w in lists:
        _, _, gl, gw = sc.oracle_group(r, l, w, 1, 0.2)
        zero_min += int(((gl == 0) & (gw == sc.DBL_MIN)).sum())
        zero_member += int(((gl == 0) & (gw > sc.DBL_MIN)).sum())
        neg_best += int(((gl >= 1) & (gw < 0)).sum())
    assert zero_min >= 3 and zero_member >= 3 and neg_best >= 3, (zero_min, zero_member, neg_best)


def _classes(rects, eps=0.2):
    """Members of each class, classes in order of first appearance."""
    sim, _ = gc.similar_matrix(rects, eps)
    n = len(rects)
    label = np.full(n, -1)
    out = []
    for i in range(n):
        if label[i] >= 0:
            continue
        todo, label[i] = [i], len(out)
        members = []
        while todo:
            a = todo.pop()
            members.append(a)
            for b in np.nonzero(sim[a] & (label < 0))[0]:
                label[b] = len(out)
                todo.append(int(b))
        out.append(sorted(members))
    return out


@pytest.mark.parametrize("which", ["haar", "lbp"])
def test_detector_frames_cover_the_cases(which, haar_xml, lbp_xml):
    """With the oracle at scaleFactor 1.1: two grouped rectangles at least on some frame and none on frame 1; more than 16
    candidates on frame 3 (the regrow tests' capacity); classes of more than two members whose best weight is neither the
    first member's nor the last's; LBP: negative and tied weights."""
    xml = haar_xml if which == "haar" else lbp_xml
    o = orc.load_cascade_xml(xml)
    frames = sc.detector_frames()
    grouped = sc.oracle_scores(xml, 2)
    assert max(len(g[0]) for g in grouped) >= 2 and len(grouped[1][0]) == 0
    assert all((g[1] == o.nstages).all() for g in grouped)
    not_first = not_last = neither = 0
    allw = []
    for f in frames:
        r, w = sc.ordered_candidates(o, f)
        allw.append(w)
        for members in _classes(r):
            if len(members) > 2:
                best = w[members].max()
                not_first += best != w[members[0]]
                not_last += best != w[members[-1]]
                neither += best != w[members[0]] and best != w[members[-1]]
    assert len(allw[1]) == 0 and len(allw[3]) > 16
    assert not_first >= 3 and not_last >= 3 and neither >= 1, (not_first, not_last, neither)
    allw = np.concatenate(allw)
    if which == "lbp":
        assert (allw < 0).sum() >= 5 and len(np.unique(allw)) < len(allw)
    else:
        assert len(np.unique(allw)) > len(allw) // 2
    # the scores in candidate order and grouped at threshold 2 are orc.detect_multiscale_levels', compared sorted
    for f, (gr, gl, gw) in zip(frames, grouped):
        wr, wl, ww = orc.detect_multiscale_levels(o, f, 1.1, 2, nthreads=8)
        a = np.lexsort((gw, gr[:, 3], gr[:, 2], gr[:, 1], gr[:, 0])) if len(gr) else np.zeros(0, int)
        b = np.lexsort((ww, wr[:, 3], wr[:, 2], wr[:, 1], wr[:, 0])) if len(wr) else np.zeros(0, int)
        assert gr.shape == wr.shape and (gr[a] == wr[b]).all() and (gl[a] == wl[b]).all() and (gw[a] == ww[b]).all()


def test_score_cascade_yields_several_weights_and_many_candidates():
    o = orc.load_cascade_xml(sc.score_cascade())
    assert o.nstages == 1
    counts, distinct = [], set()
    for f in sc.score_frames():
        r, w = sc.ordered_candidates(o, f)
        counts.append(len(r))
        distinct |= set(w.tolist())
    assert counts[0] > sc.T + 400 and 16 < counts[1] < sc.T, counts
    assert len(distinct) >= 3, distinct
    grouped = sc.oracle_scores(sc.score_cascade(), 2, "many")
    assert all(len(g[0]) >= 1 for g in grouped)
