"""cc_sample_plan (host, no device) against the numpy witness, bit for bit: doubles are compared as uint64."""
import ctypes as C
import re

import numpy as np
import pytest

from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import samples as S
from tests import sample_witness as W
from tests.sample_cases import BARCODE, BG_LIST_SIZES, CASES, EDGE_CASES, bg_images


def _bits(values):
    return np.asarray(values, np.float64).reshape(-1).view(np.uint64)


def _compare(recs, spans, want, n):
    for i in range(n):
        r, w = recs[i], want[i]
        assert (_bits(list(r.quad)) == _bits(w["quad"])).all(), ("quad", i)
        assert (_bits(list(r.coeffs)) == _bits(w["coeffs"])).all(), ("coeffs", i)
        assert (spans[i] == w["spans"]).all(), ("spans", i)
        assert (r.roi_x, r.roi_y, r.roi_w, r.roi_h) == w["roi"], ("roi", i)
        assert (r.inverse, r.forecolordev) == (w["inverse"], w["forecolordev"]), ("inverse / forecolordev", i)
        assert (r.bg_image, r.bg_w, r.bg_h, r.bg_x, r.bg_y) == w["bg"], ("bg", i)


def _run(sw, sh, ow, oh, kw, n, seed=12345):
    rng_w, rng = W.RNG(seed), S.CvRNG(seed)
    want = W.plan(sw, sh, ow, oh, W.Params(**kw), rng_w, n)
    recs, spans = S.plan(sw, sh, (ow, oh), S.SampleParams(**kw), rng, n)
    _compare(recs, spans, want, n)
    assert rng.state == rng_w.state
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_matches_witness(name):
    sw, sh, ow, oh, kw = CASES[name]
    want = _run(sw, sh, ow, oh, kw, 40)
    cw, ch = sw + 2 * (sw // 2), sh + 2 * (sh // 2)
    if name == "inscribe_clipped":  # the case is there for rectangles that leave the canvas
        assert any(r["roi"][0] == 0 or r["roi"][1] == 0 or r["roi"][0] + r["roi"][2] == cw or r["roi"][1] + r["roi"][3] == ch
                   for r in want)
    if name == "angles_0":  # axis-aligned: two topmost vertices, spans of the full object width
        assert all(r["quad"][0][1] == r["quad"][1][1] for r in want)
        assert (want[0]["spans"][sh // 2 + 1:sh // 2 + sh - 1] == [sw // 2, sw // 2 + sw]).all()
    if name == "randinv":
        assert {r["inverse"] for r in want} == {0, 1}


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_plan_matches_witness_at_edges(name):
    sw, sh, ow, oh, kw, n, seed = EDGE_CASES[name]
    _run(sw, sh, ow, oh, kw, n, seed=seed)


@pytest.mark.parametrize("seed", [2 ** 32, 2 ** 63 + 5])
def test_plan_seeds_past_32_bits(seed):
    assert S.CvRNG(seed).state == seed  # neither is folded to its low half
    _run(40, 24, 24, 24, dict(invert=W.RANDOM_INVERT), 10, seed=seed)


def _witness_planned_before_refusal(sw, sh, ow, oh, kw, seed, limit):
    """How many samples the witness plans before it refuses one as nonconvex, and those samples."""
    rng, recs = W.RNG(seed), []
    for _ in range(limit):
        try:
            recs += W.plan(sw, sh, ow, oh, W.Params(**kw), rng, 1)
        except ValueError as e:
            assert "nonconvex" in str(e)
            return recs
    raise AssertionError("the witness refused nothing")


@pytest.mark.parametrize("sw,sh,seed,count", [(2, 9, 12345, 3), (2, 9, 2, 107), (2, 40, 12345, 0)])
def test_plan_refuses_the_sample_the_witness_refuses(sw, sh, seed, count):
    kw = dict(maxxangle=1.5, maxyangle=1.5)
    want = _witness_planned_before_refusal(sw, sh, 8, 8, kw, seed, 200)
    assert len(want) == count
    with pytest.raises(L.CascadeError) as e:
        S.plan(sw, sh, (8, 8), S.SampleParams(**kw), S.CvRNG(seed), 200)
    assert e.value.status == L.CC_ERR_INVALID_ARG and "nonconvex" in str(e.value)
    assert int(re.search(r"sample (\d+):", str(e.value)).group(1)) == count
    recs, spans = S.plan(sw, sh, (8, 8), S.SampleParams(**kw), S.CvRNG(seed), count)  # exactly as many as are valid
    _compare(recs, spans, want, count)


def test_background_list_with_fit_skip_and_ladder():
    """Images exactly the window's size, as wide but taller, too narrow (skipped) and with a four-step scale ladder."""
    n = 80
    kw = dict(invert=W.RANDOM_INVERT)
    rng_w, rng = W.RNG(), S.CvRNG()
    want = W.plan(40, 24, 24, 24, W.Params(**kw), rng_w, n, W.BgReader(BG_LIST_SIZES, 24, 24))
    recs, spans = S.plan(40, 24, (24, 24), S.SampleParams(**kw), rng, n, bg_sizes=BG_LIST_SIZES)
    _compare(recs, spans, want, n)
    assert rng.state == rng_w.state
    bgs = [r["bg"] for r in want]
    assert {b[0] for b in bgs} == {0, 1, 2, 4}  # image 3 is 23 wide: never used
    assert sorted({b[1:3] for b in bgs if b[0] == 2}) == [(51, 24), (72, 33), (102, 48), (145, 67)]
    assert {b[1:] for b in bgs if b[0] == 0} == {(24, 24, 0, 0)}  # scale 1, one window, next image
    assert {b[1] for b in bgs if b[0] == 1} == {24} and len({b[4] for b in bgs if b[0] == 1}) > 1  # steps down only


def test_plan_barcode_parameters():
    _run(600, 280, 75, 32, BARCODE, 100)


def test_plan_seed_zero():
    assert S.CvRNG(0).state == 0xFFFFFFFF
    _run(40, 24, 24, 24, {}, 10, seed=0)


def test_plan_split_calls_continue_the_stream():
    p = S.SampleParams(**BARCODE)
    rng1, rng2 = S.CvRNG(), S.CvRNG()
    recs, spans = S.plan(600, 280, (75, 32), p, rng1, 100)
    ra, sa = S.plan(600, 280, (75, 32), p, rng2, 37)
    rb, sb = S.plan(600, 280, (75, 32), p, rng2, 63)
    assert rng1.state == rng2.state
    rec_bytes = C.sizeof(L.SampleRecord)
    assert bytes(recs)[:100 * rec_bytes] == bytes(ra)[:37 * rec_bytes] + bytes(rb)[:63 * rec_bytes]
    assert (spans == np.concatenate([sa, sb])).all()


def test_bow_tie_quad_is_refused():
    src, dst = np.zeros((8, 8), np.uint8), np.zeros((32, 32), np.uint8)
    bow_tie = np.array([[4, 4], [20, 20], [20, 4], [4, 20]], np.float64)
    line = np.array([[4, 4], [8, 8], [12, 12], [16, 16]], np.float64)
    for quad in (bow_tie, line):
        with pytest.raises(L.CascadeError) as e:
            S.warp_perspective(src, dst, quad)
        assert e.value.status == L.CC_ERR_INVALID_ARG and "nonconvex" in str(e.value)
    with pytest.raises(ValueError):
        W.row_spans(bow_tie.tolist(), 32, 32)


def test_background_reader_matches_witness():
    sizes = [(b.shape[1], b.shape[0]) for b in bg_images()]
    n = 150  # image 0 (70 x 52) alone gives 12 + 2 + 1 windows over its three scales: the ladder wraps many times
    rng_w, rng = W.RNG(), S.CvRNG()
    want = W.plan(40, 24, 24, 24, W.Params(), rng_w, n, W.BgReader(sizes, 24, 24))
    reader = S._BgReader(sizes)
    ra, sa = S.plan(40, 24, (24, 24), S.SampleParams(), rng, 60, _reader=reader)  # the reader's state carries over calls too
    rb, sb = S.plan(40, 24, (24, 24), S.SampleParams(), rng, n - 60, _reader=reader)
    _compare(ra, sa, want[:60], 60)
    _compare(rb, sb, want[60:], n - 60)
    assert rng.state == rng_w.state
    bgs = [r["bg"] for r in want]
    assert {b[0] for b in bgs} == {0, 1, 2}
    assert len({b[1:3] for b in bgs if b[0] == 0}) >= 3  # several steps of one image's scale ladder
    with pytest.raises(L.CascadeError):  # no image holds the window
        S.plan(40, 24, (80, 80), S.SampleParams(), S.CvRNG(), 1, bg_sizes=sizes)


def test_symbols_bind_with_declared_argtypes():
    lib = L.lib()
    for name in ("cc_sample_plan", "cc_sampler_create", "cc_sampler_destroy", "cc_sampler_set_backgrounds", "cc_sampler_render",
                 "cc_warp_perspective_u8"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES[name][0], L.SIGNATURES[name][1])
    assert C.sizeof(L.SampleRecord) == 184 and C.sizeof(L.SampleParams) == 64


def test_plan_refuses_bad_sizes():
    for sw, sh, ow, oh in ((1, 24, 24, 24), (40, 8193, 24, 24), (40, 24, 0, 24), (40, 24, 24, 4097)):
        with pytest.raises(L.CascadeError) as e:
            S.plan(sw, sh, (ow, oh), S.SampleParams(), S.CvRNG(), 1)
        assert e.value.status == L.CC_ERR_INVALID_ARG


def test_compute_entry_points_need_a_device():
    if L.lib().cc_device_count() > 0:
        pytest.skip("a device is present")
    img = np.zeros((24, 40), np.uint8)
    with pytest.raises(L.CascadeError) as e:
        S.Sampler(img)
    assert e.value.status == L.CC_ERR_NO_DEVICE
    with pytest.raises(L.CascadeError) as e:
        S.warp_perspective(img, np.zeros((48, 64), np.uint8), [[4, 4], [40, 6], [38, 30], [6, 28]])
    assert e.value.status == L.CC_ERR_NO_DEVICE


def test_read_gray_pgm_and_npy(tmp_path):
    img = np.arange(6 * 5, dtype=np.uint8).reshape(5, 6) * 7
    (tmp_path / "a.pgm").write_bytes(b"P5 # c\n6\n# another\n5 255\n" + img.tobytes())
    np.save(tmp_path / "a.npy", img)
    assert (S.read_gray(str(tmp_path / "a.pgm")) == img).all() and (S.read_gray(str(tmp_path / "a.npy")) == img).all()
    (tmp_path / "b.pgm").write_bytes(b"P2\n1 1\n255\n0\n")
    with pytest.raises(ValueError):
        S.read_gray(str(tmp_path / "b.pgm"))
    (tmp_path / "bg.txt").write_text("# list\na.npy\n\na.pgm\n")
    assert len(S.read_background_list(str(tmp_path / "bg.txt"))) == 2
