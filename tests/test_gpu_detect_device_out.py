"""cc_detect_batch_to_device against cc_detect_batch on the same frames: the rectangles left in device memory, their order
and the per-frame offsets must be exactly what the host path returns -- over several passes with a partial last one, host,
device and colour frames, the grouping thresholds, the specialised kernel, the candidate-list regrow and a short buffer.

From test_many_candidates_in_a_frame on, with the one-stage cascade of tests/group_cases.py that passes almost every window:
the order is held to the oracle's raw candidates sorted by (scale, gy, gx), frames of thousands of candidates, a pass of 300
frames, and a caller's stream with no device-wide synchronisation."""
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from oracle import oracle as orc
from tests import group_cases as gc
from tests.util import frame_natural

pytestmark = pytest.mark.gpu

W, H, N = 320, 240, 5
ORDER = [1, 3, 0, 2, 4]  # a pass that fits (the flat frame), one that overflows 16 candidates, then frames with candidates


def _paste(img, seed, ks):
    tm = np.load(os.path.join(os.path.dirname(__file__), "..", "data", "face_template_24x24.npy"))
    rng = np.random.default_rng(seed)
    out = img.copy()
    for k in ks:
        s = int(24 * k)
        y, x = int(rng.integers(0, H - s)), int(rng.integers(0, W - s))
        out[y:y + s, x:x + s] = orc.resize_linear_exact(tm, s, s)
    return out


@pytest.fixture(scope="module")
def frames():
    """Smooth noise plus pasted templates; frame 1 is flat (no window passes the variance test)."""
    f = [_paste(frame_natural(W, H, 300 + i), 40 + i, ks) for i, ks in enumerate([(1.0, 1.7, 2.6), (), (1.3, 3.0), (2.0,), (1.0, 1.5, 4.0)])]
    f[1] = np.full((H, W), 77, np.uint8)
    return np.stack(f)


@pytest.fixture(scope="module", params=["haar", "lbp"])
def xml(request, haar_xml, lbp_xml):
    return haar_xml if request.param == "haar" else lbp_xml


def test_inputs_cover_the_cases(frames, haar_xml, lbp_xml):
    """On the CPU, with the oracle: a frame with two grouped rectangles at least, frame 1 with no candidate at all, frame 3
    with more than 16 (the regrow tests' capacity; the device's raw count is at least the oracle's filtered one)."""
    for path in (haar_xml, lbp_xml):
        o = orc.load_cascade_xml(path)
        grouped = [len(orc.detect_multiscale(o, f, 1.1, 2, nthreads=8)) for f in frames]
        raw = [len(orc.detect_raw(o, f, 1.1, nthreads=8).candidates) for f in frames]
        assert max(grouped) >= 2 and grouped[1] == 0 and raw[1] == 0 and raw[3] > 16 and max(raw) > 16, (path, grouped, raw)


def _to_device(p, frames, mn, cap=4096, sf=1.1, **kw):
    import torch
    d_out = torch.full((cap + 1, 4), -7, dtype=torch.int32, device="cuda")
    d_off = torch.full((len(frames) + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fills run on torch's stream, the detector on its own
    host = kw.pop("host", None)
    total = p.detect_batch_to_device(host, sf, mn, out_ptr=d_out.data_ptr(), cap=cap, offsets_ptr=d_off.data_ptr(), **kw)
    out, off = d_out.cpu().numpy(), d_off.cpu().numpy()
    assert (out[cap:] == -7).all() and off[-1] == total
    return [out[off[i]:off[i + 1]] for i in range(len(frames))]


def _same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and (a == b).all(), (i, a, b)


@pytest.mark.parametrize("mn", [0, 2, 3])
def test_host_and_device_frames(xml, frames, mn):
    import torch
    p = cc.CascadeClassifier(xml, max_batch=2)  # 5 frames: passes of 2, 2 and 1
    want = p.detect_batch(frames, 1.1, mn)
    if mn == 2:
        assert max(len(w) for w in want) >= 2 and len(want[1]) == 0
    _same(_to_device(p, frames, mn, host=frames), want)
    t = torch.from_numpy(frames).cuda()
    _same(_to_device(p, frames, mn, device_ptr=t.data_ptr(), shape=t.shape), want)
    _same(p.detect_batch(frames, 1.1, mn), want)  # the host path on the same detector afterwards
    _same(_to_device(p, frames[:1], mn, host=frames[:1]), want[:1])  # one frame: an ordinary pass, no graph


def test_colour_frames(xml, frames):
    import torch
    bgr = np.stack([frames, np.roll(frames, 3, 2), 255 - frames], -1)
    p = cc.CascadeClassifier(xml, max_batch=2)
    want = p.detect_batch(bgr, 1.1, 2)
    _same(_to_device(p, bgr, 2, host=bgr), want)
    t = torch.from_numpy(bgr).cuda()
    _same(_to_device(p, bgr, 2, device_ptr=t.data_ptr(), shape=t.shape), want)


def test_after_specialize(xml, frames):
    p = cc.CascadeClassifier(xml, max_batch=2)
    want = p.detect_batch(frames, 1.1, 2)
    p.specialize(4)
    _same(_to_device(p, frames, 2, host=frames), want)


def test_regrow_of_the_candidate_lists(xml, frames, monkeypatch):
    want = cc.CascadeClassifier(xml, max_batch=2).detect_batch(frames, 1.1, 2)
    monkeypatch.setenv("CCAMD_CAND_CAP", "16")
    for mb in (2, 8):
        q = cc.CascadeClassifier(xml, max_batch=mb)  # fresh detector: its first call meets lists of 16 candidates
        assert q.candidate_capacity() == 16
        _same(_to_device(q, frames, 2, host=frames), want)
        grown = q.candidate_capacity()
        assert grown > 16  # a pass overflowed, was dropped on the device and redone with longer lists
        _same(_to_device(q, frames, 2, host=frames), want)  # and the grown lists
        assert q.candidate_capacity() == grown
        _same(q.detect_batch(frames, 1.1, 2), want)


def test_regrow_behind_a_pass_that_fitted(xml, frames, monkeypatch):
    """Frames in ORDER. max_batch 1: five passes of one frame; pass 0 (flat) fits, pass 1 overflows, the pass launched behind
    it is dropped on the device and redone before pass 3 is launched, with lists that its own count outgrows again.
    max_batch 2: passes of 2, 2, 1, the first overflows and the second is dead behind it."""
    perm = np.ascontiguousarray(frames[ORDER])
    want = cc.CascadeClassifier(xml, max_batch=2).detect_batch(perm, 1.1, 2)
    monkeypatch.setenv("CCAMD_CAND_CAP", "16")
    for mb in (1, 2):
        q = cc.CascadeClassifier(xml, max_batch=mb)
        assert q.candidate_capacity() == 16
        _same(_to_device(q, perm, 2, host=perm), want)
        grown = q.candidate_capacity()
        assert grown > 16
        _same(_to_device(q, perm, 2, host=perm), want)
        assert q.candidate_capacity() == grown
        _same(q.detect_batch(perm, 1.1, 2), want)


def test_frames_smaller_than_the_window(xml, frames):
    """16x16 frames under a 24x24 window: the plan has no scale, the pass returns before it has a workspace and only the
    grouping launches run. No rectangle, every offset 0, `out` untouched -- on a fresh detector and on a used one."""
    import torch
    small = np.ascontiguousarray(frames[:3, :16, :16])
    used = cc.CascadeClassifier(xml, max_batch=2)
    _to_device(used, frames, 2, host=frames)
    for p in (cc.CascadeClassifier(xml, max_batch=2), used):
        d_out = torch.full((8, 4), -7, dtype=torch.int32, device="cuda")
        d_off = torch.full((len(small) + 1,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        total = p.detect_batch_to_device(small, 1.1, 2, out_ptr=d_out.data_ptr(), cap=8, offsets_ptr=d_off.data_ptr())
        assert total == 0 and (d_off.cpu().numpy() == 0).all() and (d_out.cpu().numpy() == -7).all()


def test_cap_too_small(xml, frames):
    import torch
    p = cc.CascadeClassifier(xml, max_batch=2)
    want = p.detect_batch(frames, 1.1, 0)
    n = sum(len(w) for w in want)
    assert n > 16
    cap = n - 1
    d_out = torch.full((cap + 1, 4), -7, dtype=torch.int32, device="cuda")
    d_off = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(cc.CascadeError) as err:
        p.detect_batch_to_device(frames, 1.1, 0, out_ptr=d_out.data_ptr(), cap=cap, offsets_ptr=d_off.data_ptr())
    assert err.value.status == L.CC_ERR_BUFFER_TOO_SMALL and err.value.needed == n
    out, off = d_out.cpu().numpy(), d_off.cpu().numpy()
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert (out[:cap] == np.concatenate(want)[:cap]).all() and (out[cap] == -7).all()
    _same(p.detect_batch(frames, 1.1, 0), want)  # the failed call left no pass pending
    _same(_to_device(p, frames, 0, host=frames), want)
    with pytest.raises(cc.CascadeError) as err:
        p.detect_batch_to_device(frames, 1.1, 0, out_ptr=d_out.data_ptr(), cap=-1, offsets_ptr=d_off.data_ptr())
    assert err.value.status == L.CC_ERR_INVALID_ARG
    with pytest.raises(cc.CascadeError) as err:
        p.detect_batch_to_device(frames, 1.1, 0, out_ptr=d_out.data_ptr(), cap=cap, offsets_ptr=0)
    assert err.value.status == L.CC_ERR_INVALID_ARG


def test_after_an_uncollected_submit(xml, frames):
    p = cc.CascadeClassifier(xml, max_batch=2)
    want = p.detect_batch(frames, 1.1, 2)
    t = p.detect_batch_submit(frames, 1.1, 2)  # its last pass is still pending inside the detector
    _same(_to_device(p, frames, 2, host=frames), want)
    _same(p.detect_batch_collect(t), want)


def test_unknown_pixel_format_and_hog(frames, lbp_xml, tmp_path):
    import ctypes as C
    import torch
    from tests import hog_cascade_factory as hf
    p = cc.CascadeClassifier(lbp_xml, max_batch=2)
    d_out = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    prm = L.DetectParams(1.1, 2, 0, 0, 0, 0)
    n = C.c_int(0)
    st = L.lib().cc_detect_batch_to_device(p._detector(), frames.ctypes.data_as(C.c_void_p), 0, N, W, H, W, W * H, 99, C.byref(prm),
                                           C.c_void_p(d_out.data_ptr()), 64, C.c_void_p(d_off.data_ptr()), C.byref(n))
    assert st == L.CC_ERR_INVALID_ARG
    text, _, _ = hf.hog_cascade(np.stack([frame_natural(24, 24, k) for k in range(50)]), seed=2, stage_sizes=(2,))
    path = str(tmp_path / "hog.xml")
    open(path, "w").write(text)
    c = cc.CascadeClassifier(path)
    with pytest.raises(cc.CascadeError) as err:
        c.detect_batch_to_device(frames, 1.1, 2, out_ptr=d_out.data_ptr(), cap=64, offsets_ptr=d_off.data_ptr())
    assert err.value.status == L.CC_ERR_UNSUPPORTED and "HOG" in str(err.value)


# ------------------------------------------------------------------ ordering at scale, against the oracle
def _same_as_oracle(got, which, mn):
    want = [o[0] if mn == 0 else o[1] for o in gc.oracle_results(which)]
    _same(got, want)


@pytest.mark.parametrize("mn", [0, 2])
def test_many_candidates_in_a_frame(mn, monkeypatch):
    """Four 160x120 frames in one pass, 18 913, 2 997, 0 and 349 candidates (k_cand_rank takes 2048 per turn: ten turns, two,
    none, one), default candidate capacity. minNeighbors 0: the oracle's raw candidates sorted by (scale index, gy, gx), an
    order stated without the host path; 2: oracle.detect_multiscale. detect_batch must return the same.
    max_batch 4 alone gives four passes of one frame (a batch is cut into up to four passes so that host and device work
    overlap); with CCAMD_PIPELINE_PASSES=1 it is one pass of four, which the timings confirm."""
    monkeypatch.setenv("CCAMD_PIPELINE_PASSES", "1")
    path, _ = gc.weak_cascade()
    frames = np.asarray(gc.many_candidate_frames())
    p = cc.CascadeClassifier(path, max_batch=4)
    p.set_profiling(True)
    got = _to_device(p, frames, mn, cap=32768, host=frames)
    t = p.timings(reset=True)
    assert t["frames"] == 4 and t["eval_launches"] == 1  # one pass
    assert p.candidate_capacity() == 262144  # the default, not regrown
    _same_as_oracle(got, "many", mn)
    _same(p.detect_batch(frames, 1.1, mn), got)


def _one_call_timings(p, call):
    p.timings(reset=True)
    out = call()
    return out, p.timings(reset=True)


@pytest.mark.parametrize("mn", [0, 2])
def test_a_pass_of_300_frames(mn, monkeypatch):
    """300 frames of 40x40, a fifth of them flat: with max_batch 512 and CCAMD_PIPELINE_PASSES=1 both the device-output and
    the host path run them as one pass (frames == 300, eval_launches == 1), so k_cand_segments and k_group_offsets take a
    second turn and every front-end and cascade launch has 300 as its grid's y. Then max_batch 128: passes of 128, 128 and
    44, where k_group_offsets goes on from a running total. Every result is held to the oracle, frame by frame."""
    monkeypatch.setenv("CCAMD_PIPELINE_PASSES", "1")
    path, _ = gc.weak_cascade()
    frames = np.asarray(gc.many_small_frames())
    cap = 156 * len(frames)
    for mb, passes in ((512, 1), (128, 3)):
        p = cc.CascadeClassifier(path, max_batch=mb)
        p.set_profiling(True)
        got, t = _one_call_timings(p, lambda: _to_device(p, frames, mn, cap=cap, host=frames))
        assert t["frames"] == 300 and t["eval_launches"] == passes, t
        _same_as_oracle(got, "small", mn)
        host, t = _one_call_timings(p, lambda: p.detect_batch(frames, 1.1, mn))
        assert t["frames"] == 300 and t["eval_launches"] == passes, t
        _same_as_oracle(host, "small", mn)


@pytest.mark.parametrize("colour", [False, True])
def test_on_the_callers_stream(xml, frames, colour):
    """The use the device output is for: frames uploaded, the detector run and its result consumed on one stream of the
    caller's, with no device-wide synchronisation in between -- the detector must order itself behind the upload and the
    consumer behind the detector through the stream alone."""
    import torch
    src = np.stack([frames, np.roll(frames, 3, 2), 255 - frames], -1) if colour else frames
    p = cc.CascadeClassifier(xml, max_batch=2)
    want = p.detect_batch(src, 1.1, 2)
    cap = 4096
    pinned = torch.from_numpy(np.ascontiguousarray(src)).pin_memory()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.zeros(src.shape, dtype=torch.uint8, device="cuda")
        busy = torch.ones((4096, 4096), device="cuda")
        for _ in range(8):  # some milliseconds of work ahead of the upload: a detector that did not wait would read zeros
            busy = (busy @ busy) * (1.0 / 4096)
        t.copy_(pinned, non_blocking=True)
        d_out = torch.full((cap + 1, 4), -7, dtype=torch.int32, device="cuda")
        d_off = torch.full((len(src) + 1,), -7, dtype=torch.int32, device="cuda")
        p.set_stream(s.cuda_stream)
        total = p.detect_batch_to_device(None, 1.1, 2, out_ptr=d_out.data_ptr(), cap=cap, offsets_ptr=d_off.data_ptr(),
                                         device_ptr=t.data_ptr(), shape=t.shape)
        out_copy, off_copy = d_out.clone(), d_off.clone()  # the consumer
    s.synchronize()
    p.set_stream(None)
    out, off = out_copy.cpu().numpy(), off_copy.cpu().numpy()
    assert off[-1] == total and (out[cap:] == -7).all()
    _same([out[off[i]:off[i + 1]] for i in range(len(src))], want)
