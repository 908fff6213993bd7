"""The test mode of sample synthesis on the device (cc_sampler_render_testset, Sampler.generate_testset,
create_test_samples), byte for byte against the numpy witness (tests/testset_witness.py) over the WHOLE image, the pixels
outside the rectangle included. The inputs come from tests/testset_cases.py; that each of them reaches the edge it is there
for is asserted on the host (tests/test_testset_plan_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import samples as S
from tests import sample_witness as W
from tests import testset_witness as TW
from tests.sample_cases import CASES, obj_image
from tests.testset_cases import RENDER_CASES, render_inputs, render_witness
from tests.util import frame_natural

pytestmark = pytest.mark.gpu


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _same(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} of {want.size} bytes differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _device(shape, value):
    """A device tensor of uint8 filled with value, through a blocking copy: no kernel of torch's runs, so nothing of torch's
    stream is pending when the renderer writes on its own."""
    import torch
    t = torch.from_numpy(np.full(shape, value, np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def _same_set(got, want_images, want_samples):
    assert [(g[1], g[2], g[3]) for g in got] == [(s["rect"], s["iteration"], s["bg_index"]) for s in want_samples]
    for g, w in zip(got, want_images):
        _same(g[0], w)


def _sampler(name):
    img, bgs, kw = render_inputs(name)
    s = cc.Sampler(img, kw.get("bgcolor", 0), kw.get("bgthreshold", 80))
    s.set_backgrounds(bgs)
    return s


def _generate(name, s=None, **more):
    _, _, win, _, kw, num, maxscale, seed = RENDER_CASES[name]
    own = s is None
    s = s or _sampler(name)
    try:
        return s.generate_testset(num, win, cc.SampleParams(**kw), cc.CvRNG(seed), maxscale, **more)
    finally:
        if own:
            s.close()


@pytest.mark.parametrize("name", sorted(RENDER_CASES))
def test_testset_matches_witness(name):
    images, samples, maxscale = render_witness(name)
    got, ms = _generate(name)
    _same_set(got, images, samples)
    assert ms == maxscale


@pytest.mark.parametrize("name,max_batch", [("mixed_sizes", 1), ("mixed_sizes", 4), ("same_image_twice", 1), ("from_1x1_window", 5)])
def test_batches_equal_one_call(name, max_batch):
    images, samples, _ = render_witness(name)
    got, _ = _generate(name, max_batch=max_batch)
    _same_set(got, images, samples)


def test_split_calls_equal_one_and_restart():
    """5 + 11 iterations on one Sampler equal the witness's 16; after restart_testset the loop starts again."""
    name = "from_1x1_window"
    _, _, win, _, kw, num, maxscale, seed = RENDER_CASES[name]
    images, samples, _ = render_witness(name)
    s, rng = _sampler(name), cc.CvRNG(seed)
    a, ms = s.generate_testset(5, win, cc.SampleParams(**kw), rng, maxscale)
    b, ms = s.generate_testset(num, win, cc.SampleParams(**kw), rng, ms)  # the list ends the run after 11 more
    _same_set(a + b, images, samples)
    assert s.generate_testset(3, win, cc.SampleParams(**kw), rng, ms)[0] == []
    s.restart_testset()
    again, _ = s.generate_testset(num, win, cc.SampleParams(**kw), cc.CvRNG(seed), maxscale)
    s.close()
    _same_set(again, images, samples)


def test_device_output_equals_host_output():
    name = "equal_sizes"
    _, _, win, sizes, kw, num, maxscale, seed = RENDER_CASES[name]
    images, samples, ms_w = render_witness(name)
    cols, rows = sizes[0]
    s = _sampler(name)
    host, _ = _generate(name, s)
    s.restart_testset()
    t = _device((num, rows, cols), 7)
    got, ms = _generate(name, s, device_out=t.data_ptr())
    assert ms == ms_w and all(g[0] is None for g in got)
    assert [g[1:] for g in got] == [h[1:] for h in host]
    stack = t.cpu().numpy()
    for i in range(num):
        _same(stack[i], host[i][0])
        _same(stack[i], images[i])
    # frames further apart than they need, two at a time: the padding between them is not written
    s.restart_testset()
    fs = rows * cols + 37
    flat = _device(num * fs, 201)
    _generate(name, s, device_out=flat.data_ptr(), frame_stride=fs, max_batch=2)
    s.close()
    buf = flat.cpu().numpy().reshape(num, fs)
    for i in range(num):
        _same(buf[i, :rows * cols].reshape(rows, cols), images[i])
    assert (buf[:, rows * cols:] == 201).all()


def test_device_output_refuses_unequal_backgrounds():
    name = "odd_widths"
    _, _, win, sizes, kw, num, maxscale, seed = RENDER_CASES[name]
    images, samples, _ = render_witness(name)
    s, rng = _sampler(name), cc.CvRNG(seed)
    t = _device(num * max(w * h for w, h in sizes), 0)
    with pytest.raises(L.CascadeError) as e:
        s.generate_testset(num, win, cc.SampleParams(**kw), rng, maxscale, device_out=t.data_ptr())
    assert e.value.status == L.CC_ERR_INVALID_ARG and "one size" in str(e.value)
    assert rng.state == cc.CvRNG(seed).state and (t.cpu().numpy() == 0).all()  # nothing drawn, nothing written
    got, _ = s.generate_testset(num, win, cc.SampleParams(**kw), rng, maxscale)  # and the run starts where it would have
    s.close()
    _same_set(got, images, samples)


def _iou(a, b):
    x0, y0 = max(a[0], b[0]), max(a[1], b[1])
    x1, y1 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    inter = max(x1 - x0, 0) * max(y1 - y0, 0)
    return inter / float(a[2] * a[3] + b[2] * b[3] - inter)


def test_detector_runs_on_the_device_stack(haar_xml, repo_root):
    """What the mode is for: the face template pasted into four frames, the detector run on the stack without a host trip.
    The rectangles equal those on the host arrays, and each frame's ground truth is found."""
    tm = np.load(os.path.join(repo_root, "data", "face_template_24x24.npy"))
    bgs = [frame_natural(160, 120, 40 + i) for i in range(4)]
    kw = dict(maxxangle=0.0, maxyangle=0.0, maxzangle=0.0, maxintensitydev=0, bgthreshold=0)
    images, samples, _ = TW.generate(tm, bgs, 24, 24, W.Params(**kw), W.RNG(12345), 4, 3.0)
    s = cc.Sampler(tm, 0, 0)
    s.set_backgrounds(bgs)
    t = _device((4, 120, 160), 0)
    got, _ = s.generate_testset(4, (24, 24), cc.SampleParams(**kw), cc.CvRNG(12345), 3.0, device_out=t.data_ptr())
    s.close()
    _same(t.cpu().numpy(), np.stack(images))
    p = cc.CascadeClassifier(haar_xml, max_batch=4)
    on_device = p.detect_batch(None, 1.1, 1, device_ptr=t.data_ptr(), shape=(4, 120, 160))
    on_host = p.detect_batch(np.stack(images), 1.1, 1)
    for d, h, g in zip(on_device, on_host, got):
        assert d.shape == h.shape and (d == h).all()
        assert max(_iou(r, g[1]) for r in d.tolist()) > 0.7, (d, g[1])


def _planned(name):
    """A Sampler with the case's backgrounds, and the case's plan as the C ABI takes it: (sampler, items, records, spans)."""
    sw, sh, win, sizes, kw, num, maxscale, seed = RENDER_CASES[name]
    s = _sampler(name)
    items, recs, spans = S.plan_testset(sw, sh, win, cc.SampleParams(**kw), cc.CvRNG(seed), num, S.TestsetState(sizes, maxscale))
    its = (L.TestsetItem * len(items))(*[L.TestsetItem(*it) for it in items])
    return s, its, recs, spans


def _render_status(s, its, recs, spans, n, sizes, max_batch=0, host=True, device=None, frame_stride=0):
    """cc_sampler_render_testset as the C ABI has it: (status, host images)."""
    side = max(max(wh) for wh in sizes)  # room for any of the images
    out = [np.zeros((side, side), np.uint8) for _ in range(max(n, 0))]
    ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in out])
    st = L.lib().cc_sampler_render_testset(s._s, C.cast(its, C.c_void_p) if its is not None else None,
                                           C.cast(recs, C.c_void_p) if recs is not None else None, _vp(spans), n, max_batch,
                                           C.cast(ptrs, C.c_void_p) if host else None, device, frame_stride)
    return st, out


def _set(field, value):
    return lambda it, r: setattr(it, field, value(it) if callable(value) else value)


def _set_rec(field, value):
    return lambda it, r: setattr(r, field, value(r) if callable(value) else value)


REFUSALS = {  # one field of a valid item or record changed; three backgrounds of 70 x 52, 61 x 66, 90 x 55, the canvas 80 x 48
    "bg_image_count": _set("bg_image", 3),
    "bg_image_minus_1": _set("bg_image", -1),
    "x_negative": _set("x", -1),
    "y_negative": _set("y", -1),
    "x_past_the_edge": _set("x", lambda it: (70, 61, 90)[it.bg_image] - it.width + 1),
    "y_past_the_edge": _set("y", lambda it: (52, 66, 55)[it.bg_image] - it.height + 1),
    "width_zero": _set("width", 0),
    "height_zero": _set("height", 0),
    "width_4097": _set("width", 4097),
    "roi_x_negative": _set_rec("roi_x", -1),
    "roi_w_zero": _set_rec("roi_w", 0),
    "roi_past_right": _set_rec("roi_x", lambda r: 80 + 1 - r.roi_w),
    "roi_past_bottom": _set_rec("roi_y", lambda r: 48 + 1 - r.roi_h),
}


def test_render_refuses_items_outside_their_bounds():
    name = "same_image_twice"
    sizes = RENDER_CASES[name][3]
    images, samples, _ = render_witness(name)
    s, its, recs, spans = _planned(name)
    n = len(its)
    assert n == 3
    for label, change in REFUSALS.items():
        bad_i, bad_r = (L.TestsetItem * n)(), (L.SampleRecord * n)()
        C.memmove(bad_i, its, C.sizeof(bad_i))
        C.memmove(bad_r, recs, C.sizeof(bad_r))
        change(bad_i[1], bad_r[1])
        st, _ = _render_status(s, bad_i, bad_r, spans, n, sizes)
        assert st == L.CC_ERR_INVALID_ARG, label
    assert _render_status(s, its, recs, spans, -1, sizes)[0] == L.CC_ERR_INVALID_ARG
    assert _render_status(s, None, recs, spans, n, sizes)[0] == L.CC_ERR_INVALID_ARG
    assert _render_status(s, its, None, spans, n, sizes)[0] == L.CC_ERR_INVALID_ARG
    assert _render_status(s, its, recs, None, n, sizes)[0] == L.CC_ERR_INVALID_ARG
    assert _render_status(s, its, recs, spans, n, sizes, host=False)[0] == L.CC_ERR_INVALID_ARG  # no output at all
    ptrs = (C.c_void_p * n)(None, None, None)  # an output list with a NULL in it
    assert L.lib().cc_sampler_render_testset(s._s, C.cast(its, C.c_void_p), C.cast(recs, C.c_void_p), _vp(spans), n, 0,
                                             C.cast(ptrs, C.c_void_p), None, 0) == L.CC_ERR_INVALID_ARG
    t = _device(3 * 90 * 55, 0)  # all three items name the 90 x 55 image: a frame stride one byte short of it
    assert {it.bg_image for it in its} == {2}
    assert _render_status(s, its, recs, spans, n, sizes, host=False, device=t.data_ptr(), frame_stride=90 * 55 - 1)[0] == L.CC_ERR_INVALID_ARG
    assert (t.cpu().numpy() == 0).all()
    assert L.lib().cc_sampler_render_testset(s._s, None, None, None, 0, 0, None, None, 0) == L.CC_OK
    st, out = _render_status(s, its, recs, spans, n, sizes)  # and the sampler still works
    s.close()
    assert st == L.CC_OK
    for o, w in zip(out, images):
        _same(o.reshape(-1)[:w.size].reshape(w.shape), w)


def test_training_samples_still_equal_the_witness(tmp_path):
    """The pixel arithmetic moved into a function both kernels call: the training mode's bytes are what they were."""
    sw, sh, ow, oh, kw = CASES["default_20x13"]
    img = obj_image(sw, sh, 5)
    got = cc.create_training_samples(str(tmp_path / "a.vec"), img, 8, ow, oh, **kw)
    _same(got, W.generate(img, 8, ow, oh, W.Params(**kw), W.RNG(12345)))


def test_create_test_samples_from_the_command_line(tmp_path):
    """python -m cascadeclassifier_amd.samples -img -bg -info: the images, their names and the info file."""
    name = "randinv"
    _, _, win, sizes, kw, num, maxscale, seed = RENDER_CASES[name]
    img, bgs, _ = render_inputs(name)
    images, samples, _ = render_witness(name)
    S.write_gray(str(tmp_path / "obj.pgm"), img)
    for i, b in enumerate(bgs):
        S.write_gray(str(tmp_path / f"bg{i}.pgm"), b)
    (tmp_path / "bg.txt").write_text("".join(f"bg{i}.pgm\n" for i in range(len(bgs))))
    info = str(tmp_path / "out" / "deeper" / "info.dat")  # the directories are made, as icvMkDir does
    assert S.main(["-img", str(tmp_path / "obj.pgm"), "-bg", str(tmp_path / "bg.txt"), "-info", info, "-num", "100", "-randinv",
                   "-maxscale", str(maxscale), "-w", str(win[0]), "-h", str(win[1]), "-rngseed", str(seed)]) == 0
    entries = cc.read_info(info)
    assert [n for n, _ in entries] == ["%04d_%04d_%04d_%04d_%04d.pgm" % ((s["iteration"],) + s["rect"]) for s in samples]
    assert [r.tolist() for _, r in entries] == [[list(s["rect"])] for s in samples]
    for (n, _), want in zip(entries, images):
        _same(S.read_gray(os.path.join(os.path.dirname(info), n)), want)
    got_images, rects = cc.create_test_samples(str(tmp_path / "second.dat"), img, bgs, num, win[0], win[1], maxscale=maxscale,
                                               rngseed=seed, **kw)
    assert rects.tolist() == [list(s["rect"]) for s in samples] and open(info).read() == open(str(tmp_path / "second.dat")).read()
    for g, want in zip(got_images, images):
        _same(g, want)
