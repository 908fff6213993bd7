"""The numpy witness of the sample synthesis against the reference's recorded output (tests/golden/barcode.vec is the
expected_barcode.vec of the reference's createsamples README), and its two forms against each other."""
import numpy as np
import pytest

from tests import sample_witness as W
from tests.sample_cases import (BARCODE, CASES, COORD_CASES, COORD_DRAWS, EDGE_CASES, EDGE_SPARSE_ONLY, EDGE_TEXTURED,
                                PREPARE_PARAMS, PREPARE_SOURCES, ZERO_ANGLES, barcode_image, barcode_vec_samples, coord_record,
                                edge_inputs, edge_touches, edge_witness, obj_image, prepare_case, quad_walk, render_records,
                                stride_image)


def test_sparse_witness_reproduces_the_recorded_vec():
    got = W.generate(barcode_image(), 100, 75, 32, W.Params(**BARCODE), W.RNG(12345))
    want = barcode_vec_samples()
    assert got.shape == want.shape and (got == want).all(), f"{(got != want).sum()} of {want.size} bytes differ"


def test_dense_witness_reproduces_the_first_samples():
    got = W.generate(barcode_image(), 3, 75, 32, W.Params(**BARCODE), W.RNG(12345), dense=True)
    assert (got == barcode_vec_samples()[:3]).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_and_sparse_agree(name):
    sw, sh, ow, oh, kw = CASES[name]
    img = obj_image(sw, sh, 5, kw.get("bgcolor", 0))
    bg = np.random.RandomState(3).randint(0, 256, (6, oh, ow)).astype(np.uint8)
    a = W.generate(img, 6, ow, oh, W.Params(**kw), W.RNG(12345), backgrounds=bg, dense=True)
    b = W.generate(img, 6, ow, oh, W.Params(**kw), W.RNG(12345), backgrounds=bg)
    assert (a == b).all()
    assert len(np.unique(a)) > 8  # not a flat picture


def _edge_plan(name):
    sw, sh, ow, oh, kw, n, seed = EDGE_CASES[name]
    return W.plan(sw, sh, ow, oh, W.Params(**kw), W.RNG(seed), n), sw + 2 * (sw // 2), sh + 2 * (sh // 2)


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_case_meets_its_condition(name):
    """What a row of EDGE_CASES is for, asserted on the witness's plan and output: a row that stops covering its edge fails
    here, on the host, whatever the device does."""
    sw, sh, ow, oh, kw, n, seed = EDGE_CASES[name]
    recs, cw, ch = _edge_plan(name)
    out = W.generate(obj_image(sw, sh, 5, kw.get("bgcolor", 0)), n, ow, oh, W.Params(**kw), W.RNG(seed))
    if name in EDGE_TEXTURED:
        assert len(np.unique(out)) > 8
    if name in ("clipped_all_edges", "canvas_5"):
        assert min(edge_touches(recs, cw, ch)) >= 1
    if name == "canvas_5":
        assert (cw, ch) == (5, 5)
    if name == "canvas_4":
        assert (cw, ch) == (4, 4) and any(r["roi"] == (0, 0, 4, 4) for r in recs)
    if name == "flipped_quads":
        walks = [quad_walk(r["quad"]) for r in recs]
        assert {d for d, _ in walks} == {1, -1} and {t for _, t in walks} == {0, 1, 2, 3}
    if name == "idev_clamps":
        dev = [r["forecolordev"] for r in recs]
        assert min(dev) < -200 and max(dev) > 200
        assert (out == 0).any() and (out == 255).any()
    if name == "idev_zero":  # no draw for uniform(0, 0): the stream is one draw per sample shorter than with maxintensitydev=1
        assert all(r["forecolordev"] == 0 for r in recs)
        a, b = W.RNG(seed), W.RNG(seed)
        W.plan(sw, sh, ow, oh, W.Params(**kw), a, n)
        W.plan(sw, sh, ow, oh, W.Params(**dict(kw, maxintensitydev=1)), b, n)
        assert a.state != b.state
    if name == "wide_row":
        assert ow > 256 and -(-sw // 64) == 3
    if name == "deep_downscale":
        assert min(r["roi"][2] for r in recs) >= 40 * ow
    if name.startswith("window_"):
        assert max(ow, oh) == 4096
    if name.startswith("source_"):
        assert max(sw, sh) == 8192 and min(sw, sh) == 2


@pytest.mark.parametrize("name", sorted(set(EDGE_CASES) - set(EDGE_SPARSE_ONLY)))
def test_dense_and_sparse_agree_at_edges(name):
    sw, sh, ow, oh, kw, n, seed = EDGE_CASES[name]
    img, bg = edge_inputs(name)
    a = W.generate(img, n, ow, oh, W.Params(**kw), W.RNG(seed), backgrounds=bg, dense=True)
    assert (a == edge_witness(name)).all()


@pytest.mark.parametrize("bgcolor,fill,wrapped", [(300, 255, 44), (-5, 0, 251)])
def test_bgcolor_outside_a_byte_saturates_in_the_fills(bgcolor, fill, wrapped):
    """Mat = Scalar saturates (utility.cpp:607, :992); the mask test and de / dd take the int (:536-537, :555-556)."""
    assert W.fill_byte(bgcolor) == fill
    img = obj_image(40, 24, 5, fill)  # background pixels within 80 of bgcolor, object pixels outside
    s = img.astype(np.int64)
    inside = (bgcolor - 80 <= s) & (s <= bgcolor + 80)
    assert inside.any() and not inside.all()
    p = W.Params(bgcolor=bgcolor, bgthreshold=80, maxxangle=0.0, maxyangle=0.0, maxzangle=0.0)
    a = W.generate(img, 4, 24, 24, p, W.RNG(12345), dense=True)
    b = W.generate(img, 4, 24, 24, p, W.RNG(12345))
    assert (a == b).all()
    # zero angles: the 40 x 24 object sits in canvas rows 12..35, the 40 x 40 rectangle spans rows 4..43, so the window's
    # first and last rows are canvas fill blended (alpha 0) onto the background-less window's fill
    assert (a[:, (0, -1), :] == fill).all() and wrapped != fill
    assert len(np.unique(a)) > 8


@pytest.mark.parametrize("bgcolor,bgthreshold", PREPARE_PARAMS)
@pytest.mark.parametrize("w,h", PREPARE_SOURCES)
def test_prepare_cases_show_the_border_extension(w, h, bgcolor, bgthreshold):
    """The inputs of the device's prepare test are not vacuous: skipping the border extension changes the witness's bytes
    (with threshold 255 every pixel is background, the extension is a no-op and the output is the background)."""
    img, kw, bg, want, want_raw = prepare_case(w, h, bgcolor, bgthreshold)
    if bgthreshold == 255:
        assert (want == bg).all() and (want_raw == bg).all()
        return
    assert (want != want_raw).any()
    src, mask = W.start_distortion(img, bgcolor, bgthreshold)
    assert (mask == 0).any() and (mask == 255).any() and (src != img).sum() > 20


def test_stride_image_shows_a_read_past_the_row():
    w, h = 65, 5
    full = stride_image(w, h, 7)
    img = np.ascontiguousarray(full[:, :w])
    recs = W.plan(w, h, w, h, W.Params(**ZERO_ANGLES), W.RNG(12345), 2)
    src, mask = W.start_distortion(img, 0, 80)
    leaked = W.start_distortion(full[:, :w + 1], 0, 80)[0][:, :w]  # what a 3x3 maximum that saw the padding would give
    assert (render_records(src, mask, 0, recs, w, h) != render_records(leaked, mask, 0, recs, w, h)).any()


@pytest.mark.parametrize("name", sorted(COORD_CASES))
def test_out_of_range_coordinates_dense_and_sparse_agree(name):
    img = obj_image(40, 24, 5)
    src, mask = W.start_distortion(img, 0, 80)
    rec = coord_record(W.plan(40, 24, 24, 24, W.Params(), W.RNG(12345), 1)[0], name)
    bg = np.random.RandomState(51).randint(0, 256, (24, 24)).astype(np.uint8)
    with np.errstate(all="ignore"):
        a = W.render_dense(src, mask, 0, rec, 24, 24, bg)
        b = W.render_sparse(src, mask, 0, rec, 24, 24, bg)
    assert (a == b).all()
    assert (a != bg).any() == (name in COORD_DRAWS)  # all taps outside the source: alpha 0, the background stays
