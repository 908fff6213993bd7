"""cc_group_rectangles_device against cc_group_rectangles (the host restatement of cv::groupRectangles, itself held to
the oracle): rectangles, their order and the per-frame offsets must be identical, on hand-made lists that aim at the
device algorithm's joints -- closure of a class across wavefronts, class numbering, rounding of the averages, the two
filters, the LDS / global workspace switch (2048 rectangles per frame), empty frames and a short output buffer.

The second half (from test_random_lists_over_the_eps_grid on) judges the device by the oracle's plain n^2 groupRectangles
and by the host, on the inputs of tests/group_cases.py: an eps and threshold grid, calls of hundreds of frames, global
workspace slices at non-zero bases, one class and chains of thousands, and the same call repeated."""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from oracle import oracle as orc
from tests import group_cases as gc

pytestmark = pytest.mark.gpu


def _upload(frames):
    import torch
    frames = [np.asarray(f, np.int32).reshape(-1, 4) for f in frames]
    offs = np.zeros(len(frames) + 1, np.int32)
    offs[1:] = np.cumsum([len(f) for f in frames])
    allr = np.concatenate(frames) if frames else np.zeros((0, 4), np.int32)
    d_rects = torch.from_numpy(np.ascontiguousarray(allr)).cuda() if len(allr) else torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    return frames, d_rects, torch.from_numpy(offs).cuda()


def _device_group(frames, thr, eps=0.2, cap=None):
    """-> (status or None, total, per-frame arrays read back, offsets)"""
    import torch
    frames, d_rects, d_offs = _upload(frames)
    n_in = sum(len(f) for f in frames)
    cap = n_in if cap is None else cap
    d_out = torch.full((max(cap, 1) + 1, 4), -7, dtype=torch.int32, device="cuda")  # one guard row behind cap
    d_oo = torch.full((len(frames) + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fills run on torch's stream, the library on its own
    status, needed = None, None
    try:
        total = cc.group_rectangles_device(d_rects.data_ptr(), d_offs.data_ptr(), len(frames), thr, d_out.data_ptr(), cap,
                                           d_oo.data_ptr(), eps=eps)
    except cc.CascadeError as err:
        status, needed, total = err.status, getattr(err, "needed", None), None
    out, oo = d_out.cpu().numpy(), d_oo.cpu().numpy()
    assert (out[cap:] == -7).all(), "wrote past cap"
    return status, needed if total is None else total, out, oo


def _check(frames, thr, eps=0.2):
    frames = [np.asarray(f, np.int32).reshape(-1, 4) for f in frames]
    want = [cc.group_rectangles(f, thr, eps) for f in frames]
    status, total, out, oo = _device_group(frames, thr, eps)
    assert status is None
    w_off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    assert oo.tolist() == w_off.tolist() and total == w_off[-1]
    for i, w in enumerate(want):
        got = out[oo[i]:oo[i + 1]]
        assert got.shape == w.shape and (got == w).all(), (i, got[:8], w[:8])
    return want


def _chain(n=300):  # r_k ~ r_k+1 only: w = h = 40 -> delta 8, neighbours 5 apart, next-but-one 10 apart
    return np.array([[5 * k, 7, 40, 40] for k in range(n)], np.int32)


def _clusters(n_clusters, per, seed, cols=25):
    rng = np.random.default_rng(seed)
    c = np.arange(n_clusters)
    centres = np.stack([100 * (c % cols), 100 * (c // cols), np.full(n_clusters, 40), np.full(n_clusters, 40)], 1)
    r = np.repeat(centres, per, 0) + rng.integers(-2, 3, (n_clusters * per, 4))
    return r[rng.permutation(len(r))].astype(np.int32)


def test_empty_and_single():
    _check([np.zeros((0, 4))], 2)
    _check([], 2)  # no frame at all: offsets = [0]
    for thr in (0, 1):
        want = _check([[[3, 4, 30, 30]]], thr)
        assert len(want[0]) == (1 if thr == 0 else 0)


@pytest.mark.parametrize("thr", [0, 1])
def test_thresholds_zero_and_one(thr):
    rects = [[10, 10, 40, 40], [12, 11, 40, 40], [11, 12, 42, 42], [300, 300, 24, 24], [301, 300, 24, 24], [600, 10, 50, 50]]
    want = _check([rects], thr)
    assert len(want[0]) == (6 if thr == 0 else 2)


@pytest.mark.parametrize("order", ["index", "reversed", "shuffled"])
def test_chain_closes_over_wavefronts(order):
    r = _chain()
    assert abs(int(r[0, 0]) - int(r[-1, 0])) > 8  # the ends are not similar to each other
    if order == "reversed":
        r = r[::-1].copy()
    elif order == "shuffled":
        r = r[np.random.default_rng(5).permutation(len(r))]
    want = _check([r], 1)
    assert len(want[0]) == 1


def test_class_numbers_follow_first_appearance():
    a = [[500 + (k % 3), 20, 40, 40] for k in range(5)]  # first in the list, further right
    b = [[100 + (k % 3), 20, 40, 40] for k in range(5)]
    rects = [x for pair in zip(a, b) for x in pair]
    want = _check([rects], 2)
    assert len(want[0]) == 2 and want[0][0][0] > want[0][1][0]


def test_averages_round_half_to_even():
    # sums 21 / 2 = 10.5 -> 10 and 23 / 2 = 11.5 -> 12, in every field
    want = _check([[[10, 10, 40, 40], [11, 11, 41, 41], [211, 211, 41, 41], [212, 212, 42, 42]]], 1)
    assert want[0].tolist() == [[10, 10, 40, 40], [212, 212, 42, 42]]


def test_sums_above_two_to_the_24():
    r = [[6000001, 7000003, 1000, 1001], [6000002, 7000001, 1001, 1000], [6000004, 7000006, 1002, 1003]]
    assert sum(x[0] for x in r) > 1 << 24
    want = _check([r], 1)
    assert len(want[0]) == 1


@pytest.mark.parametrize("thr", [1, 3])
def test_class_sizes_at_the_threshold(thr):
    at = [[100 + k % 2, 100, 40, 40] for k in range(thr)]
    above = [[400 + k % 2, 100, 40, 40] for k in range(thr + 1)]
    want = _check([at + above, above + at, at, above], thr)
    assert [len(w) for w in want] == [1, 1, 0, 1]


def test_small_class_inside_a_big_one():
    def frame(n1, n2):
        return [[120 + k % 2, 120, 40, 40] for k in range(n1)] + [[100 + k % 2, 100, 100, 100] for k in range(n2)]
    cases = [(4, 5), (4, 4), (3, 4), (3, 3), (2, 2), (2, 9)]  # both sides of n2 > max(3, n1), and n1 < 3
    want = _check([frame(*c) for c in cases], 1)
    assert [len(w) for w in want] == [1, 2, 1, 2, 1, 1]


@pytest.mark.parametrize("n_clusters,per,loners", [(256, 8, 0), (256, 8, 1), (500, 12, 0)])
def test_workspace_switch_and_large_frame(n_clusters, per, loners):
    """2048 rectangles: the last size in LDS; 2049: the first in the global workspace; 6000: several hundred classes."""
    r = _clusters(n_clusters, per, seed=n_clusters + loners)
    if loners:
        r = np.concatenate([r[:1000], [[90000, 90000, 30, 30]], r[1000:]]).astype(np.int32)
    want = _check([r], 3)
    assert len(r) == n_clusters * per + loners and len(want[0]) == n_clusters


def test_seven_frames_three_of_them_empty():
    e = np.zeros((0, 4), np.int32)
    want = _check([e, _clusters(6, 5, 1), _chain(70), e, _clusters(3, 4, 2), _clusters(40, 60, 3), e], 2)
    assert [len(w) for w in want] == [0, 6, 1, 0, 3, 40, 0]


def test_cap_one_short():
    frames = [_clusters(6, 5, 1), np.zeros((0, 4), np.int32), _clusters(3, 4, 2)]
    want = [cc.group_rectangles(f, 2) for f in frames]
    n = sum(len(w) for w in want)
    status, needed, out, oo = _device_group(frames, 2, cap=n - 1)
    assert status == L.CC_ERR_BUFFER_TOO_SMALL and needed == n
    assert oo.tolist() == [0, 6, 6, 9]
    assert (out[:n - 1] == np.concatenate(want)[:n - 1]).all()


# ------------------------------------------------------------------ against the oracle, past one tile, block and LDS size
def _check_oracle(frames, thr, eps=0.2):
    """Device == oracle and device == host, frame by frame: rectangles, order, offsets. -> (oracle's results, raw bytes)"""
    frames = [np.asarray(f, np.int32).reshape(-1, 4) for f in frames]
    want = [orc.group_rectangles(f, thr, eps) for f in frames]
    status, total, out, oo = _device_group(frames, thr, eps)
    assert status is None
    w_off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    assert oo.tolist() == w_off.tolist() and total == w_off[-1]
    for i, (f, w) in enumerate(zip(frames, want)):
        got = out[oo[i]:oo[i + 1]]
        assert got.shape == w.shape and (got == w).all(), ("oracle", i, thr, eps, got[:8], w[:8])
        h = cc.group_rectangles(f, thr, eps)
        assert got.shape == h.shape and (got == h).all(), ("host", i, thr, eps, got[:8], h[:8])
    return want, out.tobytes() + oo.tobytes()


@pytest.mark.parametrize("eps", gc.EPS_GRID)
def test_random_lists_over_the_eps_grid(eps):
    """100 random lists as the 100 frames of one call per (eps, threshold): negative coordinates, rectangles that are not
    square, pairs exactly at delta, classes the inside filter removes (tests/test_group_cases_host.py holds the lists to that)."""
    for thr in gc.THRESHOLDS:
        _check_oracle(gc.random_lists(), thr, eps)


def test_rounding_in_the_inside_filter():
    names = list(gc.ROUNDING_CASES)
    want, _ = _check_oracle([gc.rounding_rects(n) for n in names], gc.ROUNDING_THRESHOLD, gc.ROUNDING_EPS)
    assert [len(w) for w in want] == [gc.ROUNDING_WANT[n] for n in names]


def test_global_workspace_slices_away_from_base_zero():
    """Frames of 2049, 5, 3000, 0, 2048 and 2500 rectangles: LDS and global-workspace frames take turns, and the slices of the
    frames of 3000 and 2500 start at rectangle 2054 and 7102 of the workspace."""
    loner = [[90000, 90000, 30, 30]]
    frames = [np.concatenate([_clusters(256, 8, 11), loner]), _clusters(1, 5, 12), _clusters(250, 12, 13), np.zeros((0, 4), np.int32),
              _clusters(256, 8, 14), _clusters(250, 10, 15)]
    assert [len(f) for f in frames] == [2049, 5, 3000, 0, 2048, 2500]
    want, _ = _check_oracle(frames, 3)
    assert [len(w) for w in want] == [256, 1, 250, 0, 256, 250]


@pytest.mark.parametrize("n_frames", [256, 257, 700])
def test_more_frames_than_one_scan_turn(n_frames):
    """k_group_offsets scans 256 frames per turn: one turn exactly, one frame into the second, and three turns."""
    _check_oracle(gc.small_frames(n_frames, n_frames), 1)


def test_700_frames_cap_one_short():
    frames = gc.small_frames(700, 700)
    want = [orc.group_rectangles(f, 1) for f in frames]
    n = sum(len(w) for w in want)
    status, needed, out, oo = _device_group(frames, 1, cap=n - 1)  # asserts that the guard row behind cap is untouched
    assert status == L.CC_ERR_BUFFER_TOO_SMALL and needed == n
    assert oo.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert (out[:n - 1] == np.concatenate(want)[:n - 1]).all()


def _union_find_case(kind, n):
    if kind == "one_class":
        return gc.one_class(n), 1
    if kind == "two_chains":
        return gc.two_chains(n), 2
    r = gc.chain(n)
    if kind == "chain_reversed":
        r = r[::-1].copy()
    elif kind == "chain_shuffled":
        r = r[np.random.default_rng(5).permutation(n)]
    return r, 1


@pytest.mark.parametrize("n", [2048, 3000])  # the workspace in LDS, and in global memory
@pytest.mark.parametrize("kind", ["one_class", "chain_index", "chain_reversed", "chain_shuffled", "two_chains"])
def test_union_find_contention_and_depth(kind, n):
    """One class of n (every pair unites), a chain of n in three orders (each rectangle similar to its neighbours only), and
    two chains that take turns in the list and must stay apart."""
    r, classes = _union_find_case(kind, n)
    want, _ = _check_oracle([r], 1)
    assert len(want[0]) == classes


def test_repeated_calls_are_byte_identical():
    """The result does not depend on the order in which threads run: five calls each, output and offsets compared as bytes."""
    for frames, thr, eps in [([_union_find_case("chain_shuffled", 3000)[0]], 1, 0.2), (gc.random_lists(), 2, 0.25)]:
        first = _check_oracle(frames, thr, eps)[1]
        for _ in range(4):
            status, _, out, oo = _device_group(frames, thr, eps)
            assert status is None and out.tobytes() + oo.tobytes() == first
