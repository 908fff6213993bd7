"""Sample synthesis on the device at the edges of its kernels, limits and checks, byte for byte against the numpy witness
(tests/sample_witness.py). The inputs come from tests/sample_cases.py; that each of them reaches the edge it is there for is
asserted on the host (tests/test_sample_witness_host.py)."""
import ctypes as C

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import samples as S
from tests import sample_witness as W
from tests.sample_cases import (COORD_CASES, EDGE_CASES, PREPARE_PARAMS, PREPARE_SOURCES, ZERO_ANGLES, bg_images, bg_list_images,
                                coord_record, edge_inputs, edge_witness, obj_image, prepare_case, rec_dict, render_records,
                                stride_image)
from tests.test_gpu_samples import QUADS

pytestmark = pytest.mark.gpu


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _same(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} of {want.size} bytes differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _render_status(s, recs, spans, n, ow, oh, backgrounds=None, max_batch=0):
    """cc_sampler_render as the C ABI has it: (status, output)."""
    out = np.zeros((max(n, 1), oh, ow), np.uint8)[:max(n, 0)]
    st = L.lib().cc_sampler_render(s._s, C.cast(recs, C.c_void_p) if recs is not None else None, _vp(spans), n, ow, oh,
                                   _vp(backgrounds), max_batch, _vp(out))
    return st, out


def _render(s, recs, spans, n, ow, oh, backgrounds=None, max_batch=0):
    st, out = _render_status(s, recs, spans, n, ow, oh, backgrounds, max_batch)
    L.check(st)
    return out


def _witness_records(recs, spans, n):
    return [rec_dict(recs[i], spans[i]) for i in range(n)]


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_generate_matches_witness_at_edges(name):
    sw, sh, ow, oh, kw, n, seed = EDGE_CASES[name]
    img, bg = edge_inputs(name)
    s = cc.Sampler(img, kw.get("bgcolor", 0), kw.get("bgthreshold", 80))
    got = s.generate(n, (ow, oh), cc.SampleParams(**kw), cc.CvRNG(seed), backgrounds=bg)
    s.close()
    _same(got, edge_witness(name))


@pytest.mark.parametrize("bgcolor,bgthreshold", PREPARE_PARAMS)
@pytest.mark.parametrize("w,h", PREPARE_SOURCES)
def test_prepare_past_one_block(w, h, bgcolor, bgthreshold):
    """Mask and border extension over several block columns and rows, with the (uchar) wrap of bgcolor - erode and
    dilate - bgcolor, a threshold of 0, one that swallows the image, and a bgcolor outside a byte."""
    img, kw, bg, want, _ = prepare_case(w, h, bgcolor, bgthreshold)
    s = cc.Sampler(img, bgcolor, bgthreshold)
    got = s.generate(2, (w, h), cc.SampleParams(**kw), cc.CvRNG(12345), backgrounds=bg)
    s.close()
    _same(got, want)


@pytest.mark.parametrize("bgcolor,fill", [(300, 255), (-5, 0)])
def test_bgcolor_outside_a_byte_saturates(bgcolor, fill):
    """No caller background: canvas and window are both filled with the saturated bgcolor (300 -> 255, -5 -> 0), the mask
    and the border extension use the int itself."""
    kw = dict(ZERO_ANGLES, bgcolor=bgcolor, bgthreshold=80)
    img = obj_image(40, 24, 5, fill)
    want = W.generate(img, 4, 24, 24, W.Params(**kw), W.RNG(12345))
    assert (want[:, (0, -1), :] == fill).all() and len(np.unique(want)) > 8
    s = cc.Sampler(img, bgcolor, 80)
    got = s.generate(4, (24, 24), cc.SampleParams(**kw), cc.CvRNG(12345))
    s.close()
    _same(got, want)


def _sampler_around(handle, w, h, bgcolor, bgthreshold):
    s = cc.Sampler.__new__(cc.Sampler)
    s.w, s.h, s.bgcolor, s.bgthreshold, s.device = w, h, bgcolor, bgthreshold, 0
    s._s, s._reader, s._reader_win = handle, None, None
    return s


def test_create_with_a_row_stride():
    w, h, pad = 65, 5, 7
    full = stride_image(w, h, pad)
    img = np.ascontiguousarray(full[:, :w])
    handle = C.c_void_p()
    L.check(L.lib().cc_sampler_create(0, _vp(full), w, h, w + pad, 0, 80, C.byref(handle)))
    strided = _sampler_around(handle, w, h, 0, 80)
    contiguous = cc.Sampler(img, 0, 80)
    p = cc.SampleParams(**ZERO_ANGLES)
    a = strided.generate(2, (w, h), p, cc.CvRNG(12345))
    b = contiguous.generate(2, (w, h), p, cc.CvRNG(12345))
    strided.close()
    contiguous.close()
    _same(a, b)
    _same(a, W.generate(img, 2, w, h, W.Params(**ZERO_ANGLES), W.RNG(12345)))


def _warp_strided(src, dst, quad, spad, dpad):
    """cc_warp_perspective_u8 with padded rows on both sides: (status, destination with its padding)."""
    sh, sw = src.shape
    dh, dw = dst.shape
    s = np.full((sh, sw + spad), 255, np.uint8)
    s[:, :sw] = src
    d = ((np.arange(dh)[:, None] * 5 + np.arange(dw + dpad)[None, :] * 11) % 253).astype(np.uint8)
    d[:, :dw] = dst
    q = np.ascontiguousarray(quad, np.float64).reshape(8)
    st = L.lib().cc_warp_perspective_u8(0, _vp(s), sw, sh, sw + spad, _vp(d), dw, dh, dw + dpad, _vp(q))
    return st, d


def _pattern(dw, dh):
    return ((np.arange(dh)[:, None] * 7 + np.arange(dw)[None, :] * 3) % 251).astype(np.uint8)


@pytest.mark.parametrize("name", sorted(QUADS))
@pytest.mark.parametrize("dw,dh", [(130, 9), (65, 70)])
def test_warp_past_one_block_with_strides(dw, dh, name):
    src = obj_image(23, 17, 21)
    quad = [[x * dw / 64.0, y * dh / 48.0] for x, y in QUADS[name]]
    pattern = _pattern(dw, dh)
    want = W.warp_perspective(src, pattern.copy(), quad)
    st, got = _warp_strided(src, pattern, quad, 5, 3)
    assert st == L.CC_OK
    _same(got[:, :dw], want)
    pad = ((np.arange(dh)[:, None] * 5 + np.arange(dw + 3)[None, :] * 11) % 253).astype(np.uint8)[:, dw:]
    assert (got[:, dw:] == pad).all()  # the destination's padding is not written
    spans = W.row_spans(quad, dw, dh)
    X = np.arange(dw)[None, :]
    outside = (X < spans[:, :1]) | (X > spans[:, 1:])
    assert (got[:, :dw][outside] == pattern[outside]).all() and outside.any() and not outside.all()
    assert (got[:, :dw][~outside] != pattern[~outside]).any()


OUTSIDE_QUADS = {
    "left": [[-50.0, 5.0], [-10.0, 8.0], [-12.0, 30.0], [-48.0, 28.0]],
    "right": [[70.0, 5.0], [110.0, 8.0], [108.0, 30.0], [72.0, 28.0]],
    "above": [[10.0, -40.0], [50.0, -37.0], [46.0, -6.0], [8.0, -9.0]],
    "below": [[10.0, 55.0], [50.0, 58.0], [46.0, 90.0], [8.0, 86.0]],
}


@pytest.mark.parametrize("name", sorted(OUTSIDE_QUADS))
def test_warp_quad_outside_the_destination_changes_nothing(name):
    src = obj_image(23, 17, 21)
    pattern = _pattern(64, 48)
    assert (W.warp_perspective(src, pattern.copy(), OUTSIDE_QUADS[name]) == pattern).all()
    st, got = _warp_strided(src, pattern, OUTSIDE_QUADS[name], 0, 0)
    assert st == L.CC_OK
    _same(got, pattern)


ROUNDING_QUADS = {
    "horizontal_edges": [[5.3, 4.2], [40.7, 4.2], [40.7, 30.6], [5.3, 30.6]],
    "half_rows": [[10.0, 3.5], [50.0, 6.5], [46.0, 40.5], [8.0, 35.5]],  # y = k + 0.5 for odd and even k: half to even
}


@pytest.mark.parametrize("name", sorted(ROUNDING_QUADS))
def test_warp_quads_that_rounding_decides(name):
    src = obj_image(23, 17, 21)
    pattern = _pattern(64, 48)
    want = W.warp_perspective(src, pattern.copy(), ROUNDING_QUADS[name])
    assert (want != pattern).any()
    _same(S.warp_perspective(src, pattern.copy(), ROUNDING_QUADS[name]), want)


def test_warp_of_a_1x1_source_is_singular():
    with pytest.raises(ValueError):
        W.perspective_coeffs(1, 1, QUADS["inside"])
    with pytest.raises(L.CascadeError) as e:
        S.warp_perspective(np.full((1, 1), 9, np.uint8), _pattern(64, 48), QUADS["inside"])
    assert e.value.status == L.CC_ERR_INVALID_ARG and "singular" in str(e.value)


@pytest.mark.parametrize("name", sorted(COORD_CASES))
def test_out_of_range_coordinates_through_caller_records(name):
    """Source coordinates beyond the source, the int range and the numbers (div = 0, infinities, NaN): every tap is guarded
    and the guard gives the reference's bytes."""
    img = obj_image(40, 24, 5)
    s = cc.Sampler(img)
    recs, spans = s.plan(1, (24, 24), cc.SampleParams(), cc.CvRNG(12345))
    want_rec = coord_record(rec_dict(recs[0], spans[0]), name)
    r = recs[0]
    r.roi_x, r.roi_y, r.roi_w, r.roi_h = want_rec["roi"]
    for i, v in enumerate(want_rec["coeffs"]):
        r.coeffs[i] = v
    spans[0] = want_rec["spans"]
    bg = np.random.RandomState(51).randint(0, 256, (1, 24, 24)).astype(np.uint8)
    got = _render(s, recs, spans, 1, 24, 24, backgrounds=bg)
    s.close()
    src, mask = W.start_distortion(img, 0, 80)
    with np.errstate(all="ignore"):
        want = render_records(src, mask, 0, [want_rec], 24, 24, bg)
    _same(got, want)


def test_max_batch_of_one():
    img = obj_image(40, 24, 5)
    bg = np.random.RandomState(61).randint(0, 256, (5, 13, 20)).astype(np.uint8)
    s = cc.Sampler(img)
    got = s.generate(5, (20, 13), cc.SampleParams(), cc.CvRNG(12345), backgrounds=bg, max_batch=1)
    s.close()
    _same(got, W.generate(img, 5, 20, 13, W.Params(), W.RNG(12345), backgrounds=bg))


def test_runs_of_one_scaled_background_cross_batches():
    sw, sh, ow, oh, kw, _, seed = EDGE_CASES["narrow_source"]
    img, bgs = obj_image(sw, sh, 5), bg_list_images()
    s = cc.Sampler(img)
    s.set_backgrounds(bgs)
    got = s.generate(9, (ow, oh), cc.SampleParams(**kw), cc.CvRNG(seed), max_batch=4)
    s.close()
    _same(got, W.generate(img, 9, ow, oh, W.Params(**kw), W.RNG(seed), bg_images=bgs))


@pytest.mark.parametrize("bgcolor", [200, 300])
def test_records_with_and_without_a_background_in_one_batch(bgcolor):
    """Every third record has no background image: its window is filled with the (saturated) bgcolor between the reader's
    windows of its neighbours."""
    n, bgs = 14, bg_list_images()
    img = obj_image(40, 24, 5, W.fill_byte(bgcolor))
    s = cc.Sampler(img, bgcolor, 80)
    s.set_backgrounds(bgs)
    recs, spans = s.plan(n, (24, 24), cc.SampleParams(bgcolor=bgcolor), cc.CvRNG(12345))
    for i in range(0, n, 3):
        recs[i].bg_image = -1
    got = _render(s, recs, spans, n, 24, 24, max_batch=5)
    s.close()
    src, mask = W.start_distortion(img, bgcolor, 80)
    want = render_records(src, mask, bgcolor, _witness_records(recs, spans, n), 24, 24, bg_images=bgs)
    _same(got, want)
    assert {recs[i].bg_image for i in range(n)} > {-1}  # both kinds are there


def test_a_sampler_reused_for_a_larger_call():
    """4 samples of 8 x 8, then 40 of 24 x 24: every per-batch buffer is freed and allocated again."""
    img = obj_image(40, 24, 5)
    r = np.random.RandomState(71)
    bg1, bg2 = r.randint(0, 256, (4, 8, 8)).astype(np.uint8), r.randint(0, 256, (40, 24, 24)).astype(np.uint8)
    s, rng, rng_w = cc.Sampler(img), cc.CvRNG(12345), W.RNG(12345)
    a = s.generate(4, (8, 8), cc.SampleParams(), rng, backgrounds=bg1)
    b = s.generate(40, (24, 24), cc.SampleParams(), rng, backgrounds=bg2)
    s.close()
    _same(a, W.generate(img, 4, 8, 8, W.Params(), rng_w, backgrounds=bg1))
    _same(b, W.generate(img, 40, 24, 24, W.Params(), rng_w, backgrounds=bg2))
    assert rng.state == rng_w.state


def test_set_backgrounds_twice():
    img, first, second = obj_image(40, 24, 5), bg_images(), bg_list_images()
    s, rng, rng_w = cc.Sampler(img), cc.CvRNG(12345), W.RNG(12345)
    s.set_backgrounds(first)
    a = s.generate(3, (24, 24), cc.SampleParams(), rng)
    s.set_backgrounds(second)
    b = s.generate(30, (24, 24), cc.SampleParams(), rng)
    s.close()
    _same(a, W.generate(img, 3, 24, 24, W.Params(), rng_w, bg_images=first))
    _same(b, W.generate(img, 30, 24, 24, W.Params(), rng_w, bg_images=second))  # a fresh reader over the second list


def test_one_sample_more_than_the_launch_cap():
    """32769 samples: the grid's y takes 32768, the last sample goes in a launch of its own."""
    n = 32769
    img = obj_image(2, 2, 5)
    s = cc.Sampler(img)
    recs, spans = s.plan(n, (2, 2), cc.SampleParams(), cc.CvRNG(12345))
    whole = _render(s, recs, spans, n, 2, 2)
    parts = _render(s, recs, spans, n, 2, 2, max_batch=5000)
    s.close()
    assert (whole == parts).all()
    assert len(np.unique(whole.reshape(n, -1), axis=0)) > 8
    src, mask = W.start_distortion(img, 0, 80)
    for i in (0, 32767, 32768):  # the plan is tied to the witness elsewhere; its records go through the witness's renderer
        _same(whole[i], W.render_sparse(src, mask, 0, rec_dict(recs[i], spans[i]), 2, 2))


def _set(field, value):
    return lambda r: setattr(r, field, value(r) if callable(value) else value)


REFUSALS = {  # one field of a valid record changed; the canvas is 80 x 48, the window 24 x 24, three background images
    "roi_x_negative": _set("roi_x", -1),
    "roi_w_zero": _set("roi_w", 0),
    "roi_past_right": _set("roi_x", lambda r: 80 + 1 - r.roi_w),
    "roi_past_bottom": _set("roi_y", lambda r: 48 + 1 - r.roi_h),
    "bg_image_count": _set("bg_image", 3),
    "bg_image_minus_2": _set("bg_image", -2),
    "bg_w_larger_than_image": _set("bg_w", 10000),
    "bg_x_past_the_edge": _set("bg_x", lambda r: r.bg_w - 24 + 1),
}


def test_render_refuses_records_outside_their_bounds():
    img, bgs = obj_image(40, 24, 5), bg_images()
    s = cc.Sampler(img)
    s.set_backgrounds(bgs)
    rng_w = W.RNG(12345)
    recs, spans = s.plan(3, (24, 24), cc.SampleParams(), cc.CvRNG(12345))
    rec_bytes = C.sizeof(L.SampleRecord)
    for name, change in REFUSALS.items():
        bad = (L.SampleRecord * 3)()
        C.memmove(bad, recs, 3 * rec_bytes)
        change(bad[1])
        st, _ = _render_status(s, bad, spans, 3, 24, 24)
        assert st == L.CC_ERR_INVALID_ARG, name
    assert _render_status(s, recs, spans, 3, 4097, 24)[0] == L.CC_ERR_INVALID_ARG
    assert _render_status(s, recs, spans, -1, 24, 24)[0] == L.CC_ERR_INVALID_ARG
    assert L.lib().cc_sampler_render(s._s, None, None, 0, 24, 24, None, 0, None) == L.CC_OK
    got = _render(s, recs, spans, 3, 24, 24)  # and the sampler still works
    s.close()
    _same(got, W.generate(img, 3, 24, 24, W.Params(), rng_w, bg_images=bgs))
