"""cc_group_rectangles_device_levels against cc_group_rectangles_levels (the host grouping with rejectLevels / levelWeights)
and the oracle's restatement, on the inputs of tests/score_cases.py: rectangles, levels, weights, their order and the
per-frame offsets must be identical -- over the eps and threshold grid, the copy-through at threshold 0, both workspace
placements of k_group_frames_scored (LDS up to T = 1536 rectangles a frame, the global workspace above), one class and chains
of more than T, hundreds of frames, a short buffer, and the same call repeated. Weights are compared with == on float64."""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from tests import group_cases as gc
from tests import score_cases as sc

pytestmark = pytest.mark.gpu

T = sc.T


def _device_group(frames, thr, eps=0.2, cap=None):
    """frames: [(rects, levels, weights)] -> (status or None, total or needed, out, out_levels, out_weights, out_offsets), the
    three outputs cap + 1 long: the last row is a sentinel, checked here."""
    import torch
    n_in = sum(len(f[0]) for f in frames)
    offs = np.zeros(len(frames) + 1, np.int32)
    offs[1:] = np.cumsum([len(f[0]) for f in frames])
    cat = [np.concatenate([f[k] for f in frames]) if n_in else np.zeros((1, 4) if k == 0 else 1, (np.int32, np.int32, np.float64)[k])
           for k in range(3)]
    d_r, d_l, d_w = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in cat)
    d_offs = torch.from_numpy(offs).cuda()
    cap = n_in if cap is None else cap
    d_out = torch.full((max(cap, 1) + 1, 4), -7, dtype=torch.int32, device="cuda")
    d_ol = torch.full((max(cap, 1) + 1,), -7, dtype=torch.int32, device="cuda")
    d_ow = torch.full((max(cap, 1) + 1,), -7.0, dtype=torch.float64, device="cuda")
    d_oo = torch.full((len(frames) + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fills run on torch's stream, the library on its own
    status = None
    try:
        total = cc.group_rectangles_device(d_r.data_ptr(), d_offs.data_ptr(), len(frames), thr, d_out.data_ptr(), cap, d_oo.data_ptr(),
                                           eps=eps, levels_ptr=d_l.data_ptr(), weights_ptr=d_w.data_ptr(),
                                           out_levels_ptr=d_ol.data_ptr(), out_weights_ptr=d_ow.data_ptr())
    except cc.CascadeError as err:
        status, total = err.status, getattr(err, "needed", None)
    out, ol, ow, oo = d_out.cpu().numpy(), d_ol.cpu().numpy(), d_ow.cpu().numpy(), d_oo.cpu().numpy()
    assert (out[cap:] == -7).all() and (ol[cap:] == -7).all() and (ow[cap:] == -7.0).all(), "wrote past cap"
    return status, total, out, ol, ow, oo


def _check(frames, thr, eps=0.2):
    """Device == oracle and device == host, frame by frame. -> (oracle's results, the device's raw bytes)"""
    frames = [(np.asarray(r, np.int32).reshape(-1, 4), np.asarray(l, np.int32), np.asarray(w, np.float64)) for r, l, w in frames]
    want = [sc.oracle_group(r, l, w, thr, eps)[1:] for r, l, w in frames]
    status, total, out, ol, ow, oo = _device_group(frames, thr, eps)
    assert status is None
    w_off = np.concatenate([[0], np.cumsum([len(w[0]) for w in want])])
    assert oo.tolist() == w_off.tolist() and total == w_off[-1]
    for i, (f, w) in enumerate(zip(frames, want)):
        got = (out[oo[i]:oo[i + 1]], ol[oo[i]:oo[i + 1]], ow[oo[i]:oo[i + 1]])
        host = cc.group_rectangles(f[0], thr, eps, levels=f[1], weights=f[2])
        for g, a, b in zip(got, w, host):
            assert g.shape == a.shape and (g == a).all(), ("oracle", i, thr, eps, g[:8], a[:8])
            assert g.shape == b.shape and (g == b).all(), ("host", i, thr, eps, g[:8], b[:8])
    return want, out.tobytes() + ol.tobytes() + ow.tobytes() + oo.tobytes()


@pytest.mark.parametrize("eps", gc.EPS_GRID)
def test_scored_lists_over_the_eps_grid(eps):
    """The 102 scored lists as the frames of one call per (eps, threshold)."""
    for thr in gc.THRESHOLDS:
        _check(sc.scored_lists(), thr, eps)


def test_hand_made_lists():
    want, _ = _check(sc.hand_made_lists(), 1)
    for (_, gl, gw), (wl, ww) in zip(want, sc.HAND_MADE_WANT):
        assert gl.tolist() == wl and gw.tolist() == ww


def test_threshold_zero_copies_all_three_through():
    frames = list(sc.scored_lists()) + [sc.with_scores(sc.clusters(40, 50, 3), 4)]  # the last one longer than T
    want, _ = _check(frames, 0)
    for f, w in zip(frames, want):
        assert all((a == b).all() for a, b in zip(f, w))
    _check(frames[:5], -1)


def test_both_workspace_placements_in_one_call():
    """Frames of T - 1, T, T + 1, 5, 0 and T + 400 rectangles: the first two and the fourth group in LDS, the third and the
    last in slices of the global workspace that start at rectangle 2 T - 1 and 3 T + 5 of it."""
    loner = [[90000, 90000, 30, 30]]
    r = [sc.clusters(307, 5, 11), sc.clusters(256, 6, 12), np.concatenate([sc.clusters(256, 6, 13), loner]).astype(np.int32),
         sc.clusters(1, 5, 14), np.zeros((0, 4), np.int32), sc.clusters(242, 8, 15)]
    assert [len(x) for x in r] == [T - 1, T, T + 1, 5, 0, T + 400]
    want, _ = _check([sc.with_scores(x, 20 + i) for i, x in enumerate(r)], 3)
    assert [len(w[0]) for w in want] == [307, 256, 256, 1, 0, 242]


@pytest.mark.parametrize("kind", ["one_class", "chain", "two_chains"])
def test_union_find_under_load_with_scores(kind):
    """One class of T (LDS: every member offers its level, those at the class's level their weight, to one word), a chain of
    T + 1 and two chains of T + 400 (global workspace), the chains shuffled."""
    if kind == "one_class":
        r, classes = gc.one_class(T), 1
    elif kind == "chain":
        r, classes = gc.chain(T + 1)[np.random.default_rng(5).permutation(T + 1)], 1
    else:
        r, classes = gc.two_chains(T + 400)[np.random.default_rng(6).permutation(T + 400)], 2
    frame = sc.with_scores(r, 31)
    want, _ = _check([frame], 1)
    assert len(want[0][0]) == classes
    for lv in want[0][1]:
        assert lv == 3  # some member of a class this large has the highest level


def test_257_frames():
    """k_group_offsets scans 256 frames per turn: one frame into the second turn."""
    frames = [sc.with_scores(f, 500 + i) for i, f in enumerate(gc.small_frames(257, 257))]
    want, _ = _check(frames, 1)
    assert sum(len(w[0]) for w in want) > 100


def test_cap_one_short():
    frames = [sc.with_scores(sc.clusters(6, 5, 1), 41), sc.with_scores(np.zeros((0, 4)), 42), sc.with_scores(sc.clusters(3, 4, 2), 43)]
    want = [sc.oracle_group(r, l, w, 2)[1:] for r, l, w in frames]
    n = sum(len(w[0]) for w in want)
    assert n == 9
    status, needed, out, ol, ow, oo = _device_group(frames, 2, cap=n - 1)  # asserts that the rows behind cap are untouched
    assert status == L.CC_ERR_BUFFER_TOO_SMALL and needed == n
    assert oo.tolist() == [0, 6, 6, 9]
    for got, k in ((out, 0), (ol, 1), (ow, 2)):
        assert (got[:n - 1] == np.concatenate([w[k] for w in want])[:n - 1]).all()


def test_argument_checks():
    import torch
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    w = torch.zeros(8, dtype=torch.float64, device="cuda")
    offs = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = dict(levels_ptr=d.data_ptr(), weights_ptr=w.data_ptr(), out_levels_ptr=d.data_ptr(), out_weights_ptr=w.data_ptr())
    for bad in (dict(good, levels_ptr=0), dict(good, weights_ptr=0), dict(good, out_levels_ptr=0), dict(good, out_weights_ptr=0)):
        with pytest.raises(cc.CascadeError) as err:
            cc.group_rectangles_device(d.data_ptr(), offs.data_ptr(), 1, 1, d.data_ptr(), 4, d.data_ptr(), **bad)
        assert err.value.status == L.CC_ERR_INVALID_ARG
    with pytest.raises(cc.CascadeError) as err:
        cc.group_rectangles_device(d.data_ptr(), offs.data_ptr(), 1, 1, d.data_ptr(), -1, d.data_ptr(), **good)
    assert err.value.status == L.CC_ERR_INVALID_ARG


def test_repeated_calls_are_byte_identical():
    """The result does not depend on the order in which threads run: five calls each, the three outputs and the offsets
    compared as bytes."""
    chain = sc.with_scores(gc.chain(T + 1)[np.random.default_rng(5).permutation(T + 1)], 31)
    for frames, thr, eps in [([chain], 1, 0.2), (list(sc.scored_lists()[:100]), 2, 0.25)]:
        first = _check(frames, thr, eps)[1]
        for _ in range(4):
            status, _, out, ol, ow, oo = _device_group(frames, thr, eps)
            assert status is None and out.tobytes() + ol.tobytes() + ow.tobytes() + oo.tobytes() == first
