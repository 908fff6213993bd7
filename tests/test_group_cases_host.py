"""CPU side of tests/group_cases.py: the host grouping (sort-and-sweep) against the oracle's plain n^2 restatement over the
eps and threshold grid, and checks that the shared inputs reach the cases the GPU tests rely on them for."""
import numpy as np

import cascadeclassifier_amd as cc
from oracle import oracle as orc
from tests import group_cases as gc


def test_host_grouping_matches_the_oracle_over_the_grid():
    lists = gc.random_lists()
    assert len(lists) >= 100
    assert min(len(r) for r in lists) < 10 and max(len(r) for r in lists) > 180
    assert min(int(r[:, :2].min()) for r in lists if len(r)) < 0 and any((r[:, 2] != r[:, 3]).any() for r in lists)
    for k, r in enumerate(lists):
        for eps in gc.EPS_GRID:
            for thr in gc.THRESHOLDS:
                a, b = cc.group_rectangles(r, thr, eps), orc.group_rectangles(r, thr, eps)
                assert a.shape == b.shape and (a == b).all(), (k, eps, thr)


def test_random_lists_hold_pairs_exactly_at_delta():
    """At least a tenth of the (list, eps) cases hold a similar pair with one of its four distances equal to delta."""
    cases = [(r, eps) for r in gc.random_lists() for eps in gc.EPS_GRID]
    hits = sum(gc.has_pair_at_delta(r, eps) for r, eps in cases)
    assert 10 * hits >= len(cases), (hits, len(cases))


def test_random_lists_make_the_inside_filter_remove_classes():
    """In at least a tenth of the (list, eps, threshold) cases the output is shorter than the number of classes above the
    threshold: the inside-a-bigger-class filter removed one."""
    hits = cases = 0
    for r in gc.random_lists():
        for eps in gc.EPS_GRID:
            sizes = gc.class_sizes(r, eps)
            assert sizes.sum() == len(r)
            for thr in gc.THRESHOLDS:
                cases += 1
                hits += len(orc.group_rectangles(r, thr, eps)) < int((sizes > thr).sum())
    assert 10 * hits >= cases, (hits, cases)


def test_rounding_cases_tell_the_roundings_apart():
    """r2.width * eps is exactly 2.5 (-> 2) and 3.5 (-> 4): the oracle's output has the length half-to-even gives, which is
    not what v + 0.5 truncated gives at 2.5 nor what rounding down gives at 3.5. The host agrees with the oracle."""
    eps, thr = gc.ROUNDING_EPS, gc.ROUNDING_THRESHOLD
    for name, classes in gc.ROUNDING_CASES.items():
        big = classes[0][0]
        assert big[2] * eps == float(name)
        r = gc.rounding_rects(name)
        sim, _ = gc.similar_matrix(r, eps)
        assert not sim[0, -1] and (gc.class_sizes(r, eps) == [4, 2]).all()  # the two classes stay apart
        want = orc.group_rectangles(r, thr, eps)
        assert len(want) == gc.ROUNDING_WANT[name] == gc.filter_count(classes, thr, eps, gc.round_half_even)
        got = cc.group_rectangles(r, thr, eps)
        assert got.shape == want.shape and (got == want).all()
    assert gc.filter_count(gc.ROUNDING_CASES["2.5"], thr, eps, gc.round_half_up) != gc.ROUNDING_WANT["2.5"]
    assert gc.filter_count(gc.ROUNDING_CASES["3.5"], thr, eps, gc.round_down) != gc.ROUNDING_WANT["3.5"]


def test_union_find_inputs():
    n = 3000  # the lists of 2048 are the first 2048 of these
    assert (gc.one_class(2048) == gc.one_class(n)[:2048]).all() and (gc.two_chains(2048) == gc.two_chains(n)[:2048]).all()
    i = np.arange(n)
    apart = np.abs(i[:, None] - i[None, :])
    assert gc.similar_matrix(gc.one_class(n), 0.2)[0].all()
    assert (gc.similar_matrix(gc.chain(n), 0.2)[0] == (apart <= 1)).all()  # neighbours only
    assert (gc.similar_matrix(gc.two_chains(n), 0.2)[0] == ((apart <= 2) & (apart % 2 == 0))).all()
    assert len(orc.group_rectangles(gc.two_chains(n), 1)) == 2 and len(orc.group_rectangles(gc.two_chains(2048), 1)) == 2


def test_small_frame_lists():
    for n in (256, 257, 700):
        frames = gc.small_frames(n, n)
        sizes = np.array([len(f) for f in frames])
        assert len(frames) == n and sizes.max() == 12 and n / 4 < (sizes == 0).sum() < n / 2
        assert (sizes[:256] == 0).any() and (sizes[-44:] == 0).any()
        out = [len(orc.group_rectangles(f, 1)) for f in frames]
        assert max(out) >= 3 and sum(out) > n / 2


def test_detector_inputs_cover_the_cases():
    """With the oracle and the cascade that passes almost every window, scaleFactor 1.1. The 160x120 batch: more than 4096
    candidates, between 2049 and 4096, none, a few hundred. The 40x40 batch: 300 frames, about a fifth flat with no
    candidate, frames 0 and 299 among them, and candidates in every other one."""
    many = gc.oracle_results("many")
    raw = [len(o) for o, _ in many]
    assert raw[0] == 18913 and 2049 <= raw[1] <= 4096 and raw[2] == 0 and 200 <= raw[3] <= 500, raw
    assert [len(g) for _, g in many] == [1, 2, 0, 2]
    small = gc.oracle_results("small")
    raw = np.array([len(o) for o, _ in small])
    flat = np.array([gc.small_flat(i) for i in range(gc.SMALL_N)])
    assert len(raw) == 300 and flat[0] and flat[299] and 50 <= flat.sum() <= 70
    assert (raw[flat] == 0).all() and (raw[~flat] == 156).all()
    assert all(len(g) == (0 if f else 1) for (_, g), f in zip(small, flat))
