"""cc_testset_plan (host, no device) against the numpy witness of cvCreateTestSamples (tests/testset_witness.py), bit for
bit; the conditions the shared cases exist for; dense against sparse witness; the info file and the command line."""
import ctypes as C
import re

import numpy as np
import pytest

from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import samples as S
from tests import sample_witness as W
from tests import testset_witness as TW
from tests.test_sample_plan_host import _compare
from tests.testset_cases import (DRAWS_PER_SAMPLE, PLAN_CASES, REFUSAL_ITERATION, REFUSAL_SEED, REFUSAL_SIZES, RENDER_CASES,
                                 SIZES_MIXED, SKIP_SEED, SKIP_SIZES, CountingRNG, render_inputs, render_witness)

SW, SH = 40, 24


def _product(sizes, win, kw, seed, maxscale, chunks, sw=SW, sh=SH):
    """plan_testset in calls of chunks[0], chunks[1], ... iterations: (items, records, spans, rng, state)."""
    rng, st = S.CvRNG(seed), S.TestsetState(sizes, maxscale)
    items, recs, spans = [], [], []
    for num in chunks:
        it, r, sp = S.plan_testset(sw, sh, win, S.SampleParams(**kw), rng, num, st)
        items += it
        recs += [r[i] for i in range(len(it))]
        spans += list(sp)
    return items, recs, spans, rng, st


def _same_plan(sizes, win, kw, seed, maxscale, chunks, sw=SW, sh=SH):
    rng_w, reader = CountingRNG(seed), TW.new_reader(sizes)
    want, ms_w, done_w = TW.plan(sw, sh, win[0], win[1], W.Params(**kw), rng_w, sum(chunks), reader, maxscale)
    items, recs, spans, rng, st = _product(sizes, win, kw, seed, maxscale, chunks, sw, sh)
    assert items == [(s["iteration"], s["bg_index"]) + s["rect"] for s in want]
    _compare(recs, spans, [s["rec"] for s in want], len(want))
    assert rng.state == rng_w.state
    assert np.float64(st.maxscale).view(np.uint64) == np.float64(ms_w).view(np.uint64)
    assert st.iterations == done_w == min(sum(chunks), len(sizes))
    assert (st.reader.c.last, st.reader.c.round) == (reader.last, reader.round)
    return want, rng_w, ms_w


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_plan_matches_witness(name):
    win, sizes, kw, num, maxscale, seed = PLAN_CASES[name]
    want, rng_w, ms = _same_plan(sizes, win, kw, seed, maxscale, [num])
    assert len(want) == min(num, len(sizes))  # nothing skipped in these cases
    if name.startswith("auto") or name.startswith("seed"):
        first = sizes[want[0]["bg_index"]]  # 0.7 of the first image drawn, in float, and kept
        assert ms == float(min(np.float32(0.7) * np.float32(first[0]) / np.float32(win[0]),
                               np.float32(0.7) * np.float32(first[1]) / np.float32(win[1])))
        assert len({s["bg_index"] for s in want}) > 3 and ms > 1.0
    if name == "maxscale_1":  # every rectangle is the window, and the float draw is still spent
        assert all(s["rect"][2:] == win for s in want) and rng_w.draws == DRAWS_PER_SAMPLE * len(want)
    if name == "maxscale_2.5":
        assert all(24 <= s["rect"][2] < 60 for s in want) and len({s["rect"][2] for s in want}) > 4
    if name == "randinv":
        assert {s["rec"]["inverse"] for s in want} == {0, 1} and rng_w.draws == (DRAWS_PER_SAMPLE + 1) * len(want)
    if name == "sides_of_9":  # images with a side of 9 are drawn again: more draws than the samples account for
        assert rng_w.draws > DRAWS_PER_SAMPLE * len(want) and all(min(sizes[s["bg_index"]]) >= 10 for s in want)
    if name == "num_clamped":
        assert num > len(sizes) == len(want)


@pytest.mark.parametrize("name", sorted(RENDER_CASES))
def test_plan_matches_witness_on_render_cases(name):
    sw, sh, win, sizes, kw, num, maxscale, seed = RENDER_CASES[name]
    _same_plan(sizes, win, kw, seed, maxscale, [num], sw, sh)


@pytest.mark.parametrize("chunks", [[3, 5], [1, 1, 6], [0, 8], [5, 50]])
def test_split_calls_equal_one(chunks):
    win, sizes, kw, _, maxscale, seed = PLAN_CASES["randinv"]
    whole = _product(sizes, win, kw, seed, maxscale, [8])
    parts = _product(sizes, win, kw, seed, maxscale, chunks)
    rec_bytes = C.sizeof(L.SampleRecord)
    assert whole[0] == parts[0] and len(whole[0]) == 8
    assert [bytes(r)[:rec_bytes] for r in whole[1]] == [bytes(r)[:rec_bytes] for r in parts[1]]
    assert all((a == b).all() for a, b in zip(whole[2], parts[2]))
    assert whole[3].state == parts[3].state and whole[4].maxscale == parts[4].maxscale and parts[4].iterations == 8
    _same_plan(sizes, win, kw, seed, maxscale, chunks)
    _same_plan(PLAN_CASES["auto"][1], (24, 24), {}, 12345, -1.0, [4, 8])  # the automatic maxscale is carried, not taken again


def test_a_call_after_the_list_is_used_up_does_nothing():
    rng, st = S.CvRNG(), S.TestsetState(SIZES_MIXED, 2.5)
    S.plan_testset(SW, SH, (24, 24), S.SampleParams(), rng, 8, st)
    state = rng.state
    items, _, spans = S.plan_testset(SW, SH, (24, 24), S.SampleParams(), rng, 3, st)
    assert items == [] and len(spans) == 0 and rng.state == state and st.iterations == 8


def test_sticky_skip_emits_nothing():
    n = len(SKIP_SIZES)
    rng_w, reader = CountingRNG(SKIP_SEED), TW.new_reader(SKIP_SIZES)
    want, ms, done = TW.plan(SW, SH, 24, 24, W.Params(), rng_w, n, reader)
    first = TW.new_reader(SKIP_SIZES)
    first._next_image(W.RNG(SKIP_SEED))
    assert SKIP_SIZES[first.last] == (14, 11) and 0.0 < ms < 1.0  # the first image drawn is too small, and that sticks
    assert want == [] and done == n and rng_w.draws == n  # one background draw per iteration, nothing else
    assert any(min(w, h) * 0.7 >= 24 for w, h in SKIP_SIZES)  # images that would have held a sample were there
    _same_plan(SKIP_SIZES, (24, 24), {}, SKIP_SEED, -1.0, [n])
    _same_plan(SKIP_SIZES, (24, 24), {}, SKIP_SEED, -1.0, [1, n - 1])


def _state(rng, st):
    return rng.state, st.maxscale, st.iterations, bytes(st.reader.c)


def test_rectangle_outside_its_image_is_refused():
    first = TW.new_reader(REFUSAL_SIZES)
    first._next_image(W.RNG(REFUSAL_SEED))
    assert REFUSAL_SIZES[first.last] == (400, 300)
    with pytest.raises(ValueError) as ew:
        TW.plan(SW, SH, 24, 24, W.Params(), W.RNG(REFUSAL_SEED), 4, TW.new_reader(REFUSAL_SIZES))
    assert str(ew.value).startswith(f"iteration {REFUSAL_ITERATION}: the rectangle leaves")
    rng, st = S.CvRNG(REFUSAL_SEED), S.TestsetState(REFUSAL_SIZES)
    before = _state(rng, st)
    with pytest.raises(L.CascadeError) as e:
        S.plan_testset(SW, SH, (24, 24), S.SampleParams(), rng, 4, st)
    assert e.value.status == L.CC_ERR_INVALID_ARG
    assert int(re.search(r"iteration (\d+):", str(e.value)).group(1)) == REFUSAL_ITERATION and "leaves" in str(e.value)
    assert _state(rng, st) == before
    # the iterations before the refused one are planned as the witness plans them, and the state moves on from there
    want, _, _ = TW.plan(SW, SH, 24, 24, W.Params(), W.RNG(REFUSAL_SEED), REFUSAL_ITERATION - 1, TW.new_reader(REFUSAL_SIZES))
    items, recs, spans = S.plan_testset(SW, SH, (24, 24), S.SampleParams(), rng, REFUSAL_ITERATION - 1, st)
    assert items == [(s["iteration"], s["bg_index"]) + s["rect"] for s in want] and len(items) == REFUSAL_ITERATION - 1
    assert st.maxscale == 8.75
    moved = _state(rng, st)
    with pytest.raises(L.CascadeError):
        S.plan_testset(SW, SH, (24, 24), S.SampleParams(), rng, 1, st)
    assert _state(rng, st) == moved


def test_every_image_under_10_pixels_is_refused():
    sizes = [(9, 50), (50, 9), (9, 9)]
    with pytest.raises(ValueError):
        TW.plan(SW, SH, 24, 24, W.Params(), W.RNG(), 3, TW.new_reader(sizes), 1.0)
    rng, st = S.CvRNG(), S.TestsetState(sizes, 1.0)
    before = _state(rng, st)
    with pytest.raises(L.CascadeError) as e:
        S.plan_testset(SW, SH, (24, 24), S.SampleParams(), rng, 3, st)
    assert e.value.status == L.CC_ERR_INVALID_ARG and "iteration 1:" in str(e.value) and _state(rng, st) == before


def test_plan_refuses_what_the_training_plan_refuses():
    for sw, sh, win in ((1, 24, (24, 24)), (40, 8193, (24, 24)), (40, 24, (0, 24)), (40, 24, (24, 4097))):
        with pytest.raises(L.CascadeError) as e:
            S.plan_testset(sw, sh, win, S.SampleParams(), S.CvRNG(), 1, S.TestsetState(SIZES_MIXED, 1.0))
        assert e.value.status == L.CC_ERR_INVALID_ARG
    with pytest.raises(L.CascadeError) as e:  # the scaled window passes 4096
        S.plan_testset(SW, SH, (24, 24), S.SampleParams(), S.CvRNG(), 1, S.TestsetState([(16000, 16000)], 1e6))
    assert e.value.status == L.CC_ERR_INVALID_ARG and "iteration 1:" in str(e.value)
    with pytest.raises(ValueError):
        TW.plan(SW, SH, 24, 24, W.Params(), W.RNG(), 1, TW.new_reader([(16000, 16000)]), 1e6)
    with pytest.raises(L.CascadeError) as e:  # a 2 x 40 source at these angles: the first quad is nonconvex
        S.plan_testset(2, 40, (8, 8), S.SampleParams(maxxangle=1.5, maxyangle=1.5), S.CvRNG(), 1, S.TestsetState(SIZES_MIXED, 1.0))
    assert e.value.status == L.CC_ERR_INVALID_ARG and "nonconvex" in str(e.value) and "iteration 1:" in str(e.value)
    with pytest.raises(L.CascadeError):
        S.plan_testset(SW, SH, (24, 24), S.SampleParams(), S.CvRNG(), -1, S.TestsetState(SIZES_MIXED, 1.0))


def test_float_uniform_is_one_draw_in_float():
    rng = W.RNG(12345)
    v = TW.uniform_float(rng, 1.0, np.float32(8.75))
    ref = W.RNG(12345)
    t = ref.next()
    assert rng.state == ref.state  # one draw
    f = np.float32(t) * np.float32(2.0) ** -32
    assert v.dtype == np.float32 and v == np.float32(np.float32(f * np.float32(7.75)) + np.float32(1.0)) and 1.0 <= v < 8.75
    assert float(v) != t * 2.0 ** -32 * 7.75 + 1.0  # a value the double arithmetic does not give


@pytest.mark.parametrize("name", sorted(RENDER_CASES))
def test_render_case_meets_its_condition(name):
    _, _, win, sizes, kw, num, _, _ = RENDER_CASES[name]
    images, samples, ms = render_witness(name)
    rects = [s["rect"] for s in samples]
    areas = [r[2] * r[3] for r in rects]
    assert len(samples) == num
    for s, img in zip(samples, images):  # outside the rectangle the image is its background, inside it is not
        x, y, w, h = s["rect"]
        bg = render_inputs(name)[1][s["bg_index"]]
        outside = np.ones(bg.shape, bool)
        outside[y:y + h, x:x + w] = False
        # (a rectangle of a few pixels can lie under a mask of 0: the inscribed rectangle's corners are outside the quad)
        assert (img[outside] == bg[outside]).all() and (w * h < 25 or (img[~outside] != bg[~outside]).any())
    if name == "rect_256":
        assert set(areas) == {256}
    if name == "rect_257_row":
        assert set(rects[i][2:] for i in range(num)) == {(257, 1)}
    if name == "from_1x1_window":
        assert {r[2] for r in rects} == set(range(1, 8)) and all(r[2] == r[3] for r in rects)
    if name == "whole_image":
        assert set(rects) == {(0, 0, 10, 10)}
    if name == "odd_widths":
        assert sum(sizes[s["bg_index"]][0] % 4 != 0 for s in samples) >= 4
    if name == "mixed_sizes":
        assert min(areas) <= 25 * 16 and max(areas) >= 280 * 185
    if name == "same_image_twice":
        assert len({s["bg_index"] for s in samples}) < num
    if name == "randinv":
        assert {s["rec"]["inverse"] for s in samples} == {0, 1}
    if name == "idev_clamps":
        devs = [s["rec"]["forecolordev"] for s in samples]
        assert min(devs) < -155 and max(devs) > 155  # object pixels of 100..199 clamp on both sides
    if name == "equal_sizes":
        assert ms == float(np.float32(0.7) * np.float32(96) / np.float32(24)) and len({s["bg_index"] for s in samples}) > 2


@pytest.mark.parametrize("name", sorted(RENDER_CASES))
def test_dense_and_sparse_witness_agree(name):
    _, _, _, _, kw, _, _, _ = RENDER_CASES[name]
    img, bgs, _ = render_inputs(name)
    images, samples, _ = render_witness(name)
    dense = TW.render(img, bgs, W.Params(**kw), samples, dense=True)
    assert all((a == b).all() for a, b in zip(dense, images))


def test_info_file_round_trip(tmp_path):
    entries = [("0001_0012_0003_0043_0043.pgm", [(12, 3, 43, 43)]), ("two.pgm", [(1, 2, 3, 4), (50, 60, 70, 80)]), ("none.pgm", [])]
    path = str(tmp_path / "info.dat")
    S.write_info(path, entries)
    assert open(path).read() == ("0001_0012_0003_0043_0043.pgm 1 12 3 43 43\ntwo.pgm 2 1 2 3 4 50 60 70 80\nnone.pgm 0\n")
    got = S.read_info(path)
    assert [n for n, _ in got] == [n for n, _ in entries]
    assert all(r.shape == (len(w), 4) and r.dtype == np.int32 and r.tolist() == [list(x) for x in w] for (_, r), (_, w) in zip(got, entries))
    (tmp_path / "bad.dat").write_text("a.pgm 2 1 2 3 4\n")
    with pytest.raises(ValueError):
        S.read_info(str(tmp_path / "bad.dat"))


def test_write_gray_round_trip(tmp_path):
    img = (np.arange(7 * 5, dtype=np.uint8).reshape(5, 7) * 9)
    S.write_gray(str(tmp_path / "a.pgm"), img)
    assert (S.read_gray(str(tmp_path / "a.pgm")) == img).all()
    img[0, 0] = 10  # a pixel that is a line feed right behind the header
    S.write_gray(str(tmp_path / "b.pgm"), img)
    assert (S.read_gray(str(tmp_path / "b.pgm")) == img).all()


def test_command_line_selects_the_mode():
    mode, a = S.parse_args(["-img", "o.pgm", "-vec", "out.vec", "-num", "7"])
    assert mode == "training" and (a.vec, a.num, a.info) == ("out.vec", 7, None)
    mode, a = S.parse_args(["-img", "o.pgm", "-bg", "bg.txt", "-info", "out/info.dat", "-maxscale", "3.5", "-w", "20", "-h", "13"])
    assert mode == "test" and (a.info, a.bg, a.maxscale, a.w, a.h) == ("out/info.dat", "bg.txt", 3.5, 20, 13)
    assert S.parse_args(["-img", "o.pgm", "-bg", "bg.txt", "-info", "i.dat"])[1].maxscale == -1.0  # the tool's default
    # -img with -vec is the training mode whatever else is given (createsamples.cpp:184 comes first)
    assert S.parse_args(["-img", "o.pgm", "-vec", "out.vec", "-bg", "bg.txt", "-info", "i.dat"])[0] == "training"
    for argv in (["-img", "o.pgm"], ["-img", "o.pgm", "-info", "i.dat"], ["-img", "o.pgm", "-bg", "bg.txt"], ["-vec", "out.vec"]):
        with pytest.raises(SystemExit):
            S.parse_args(argv)


def test_symbols_bind_with_declared_argtypes():
    lib = L.lib()
    for name in ("cc_testset_plan", "cc_sampler_render_testset"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES[name][0], L.SIGNATURES[name][1])
    assert C.sizeof(L.TestsetItem) == 24
