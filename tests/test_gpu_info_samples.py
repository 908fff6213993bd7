"""The -info mode on the device (cc_resize_area_u8, cc_samples_from_info, create_samples_from_info), byte for byte against
the numpy witness (tests/area_witness.py). The inputs come from tests/info_cases.py; that each of them reaches the edge it is
there for is asserted on the host (tests/test_area_witness_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import samples as S
from cascadeclassifier_amd.detector import vec_read
from tests import area_witness as AW
from tests.info_cases import (INFO_CASES, NO_OVERFLOW_SIDES, OVERFLOW_SIDES, RECORD_REFUSALS, RESIZE_CASES, info_case, info_want,
                              random_image, resize_input, resize_want)
from tests.sample_cases import obj_image
from tests.util import frame_natural

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("name", sorted(RESIZE_CASES))
def test_resize_area_matches_witness(name):
    _, _, dw, dh = RESIZE_CASES[name]
    _same(cc.resize_area(resize_input(name), dw, dh), resize_want(name))


@pytest.mark.parametrize("name", ["3x2_fast", "25_to_24", "27x29_to_5x7", "row_301", "2x2_fast"])
def test_resize_area_with_a_source_stride(name):
    """The source is a view of a wider array of 255: nothing of the padding may be read."""
    sw, sh, dw, dh = RESIZE_CASES[name]
    wide = np.full((sh, sw + 13), 255, np.uint8)
    wide[:, :sw] = resize_input(name)
    view = wide[:, :sw]
    assert view.strides == (sw + 13, 1)
    _same(cc.resize_area(view, dw, dh), resize_want(name))


def test_resize_area_just_under_the_overflow_limit():
    """4096 x 2056 to 1 x 1: the largest integer-ratio block whose sum stays below 2^31, all 255 and random."""
    w, h = NO_OVERFLOW_SIDES
    for img in (np.full((h, w), 255, np.uint8), random_image(w, h, 41)):
        _same(cc.resize_area(img, 1, 1), AW.resize_area(img, 1, 1))


@pytest.mark.parametrize("name", INFO_CASES)
def test_samples_match_witness(name):
    images, records, win = info_case(name)
    _same(cc.samples_from_info(images, records, win), info_want(name))


@pytest.mark.parametrize("name,max_batch", [("mixed", 1), ("mixed", 4), ("corners", 3), ("window_5x7", 2)])
def test_batches_equal_one_call(name, max_batch):
    """max_batch = 4 cuts "mixed" between records 7 and 8, 3 cuts "corners" inside image 0's records: the image is uploaded
    again for the next batch."""
    images, records, win = info_case(name)
    _same(cc.samples_from_info(images, records, win, max_batch=max_batch), info_want(name))


def test_strided_images_in_the_info_layer():
    images, records, win = info_case("mixed")
    wide = []
    for im in images:
        w = np.full((im.shape[0], im.shape[1] + 7), 255, np.uint8)
        w[:, :im.shape[1]] = im
        wide.append(w[:, :im.shape[1]])
    _same(cc.samples_from_info(wide, records, win), info_want("mixed"))


def test_device_output_equals_host_output():
    images, records, win = info_case("mixed")
    want = info_want("mixed")
    n, (dw, dh) = len(records), win
    t = _device((n + 1, dh, dw), 201)
    assert cc.samples_from_info(images, records, win, device_out=t.data_ptr(), host=False) is None
    got = t.cpu().numpy()
    _same(got[:n], want)
    assert (got[n] == 201).all()  # nothing past the n windows is written
    t = _device((n, dh, dw), 7)  # both outputs, in batches of 4
    host = cc.samples_from_info(images, records, win, device_out=t.data_ptr(), max_batch=4)
    _same(host, want)
    _same(t.cpu().numpy(), want)


def test_barcode_info(tmp_path, repo_root):
    """The reference's own input of this mode, through create_samples_from_info and the command line. The info file names a
    .png; the gray pixels are stored under that name as a binary PGM, which read_gray tells by its magic number."""
    gray = resize_input("barcode")
    info = str(tmp_path / "barcode.info")
    open(info, "w").write(open(os.path.join(repo_root, "tests", "golden", "barcode.info")).read())
    S.write_gray(str(tmp_path / "ean13_5012345678900.png"), gray)
    vec = str(tmp_path / "out.vec")
    out = cc.create_samples_from_info(vec, info, num=1, w=75, h=32)
    _same(out, resize_want("barcode")[None])
    _same(vec_read(vec).reshape(1, 32, 75), out)
    assert np.frombuffer(open(vec, "rb").read(8), np.int32).tolist() == [1, 75 * 32]
    assert S.main(["-info", info, "-vec", str(tmp_path / "cli.vec"), "-w", "75", "-h", "32", "-num", "1"]) == 0
    assert open(str(tmp_path / "cli.vec"), "rb").read() == open(vec, "rb").read()
    out = cc.create_samples_from_info(vec, info)  # the tool's defaults: 24 x 24, and the file ends the run
    _same(out, AW.samples([gray], [(0, 0, 0, 600, 280)], 24, 24))


def test_round_trip_with_create_test_samples(tmp_path):
    """create_test_samples writes images and info.dat; create_samples_from_info on that file gives what the witness gives
    on the returned images and rectangles."""
    obj = obj_image(40, 24, 5)
    bgs = [frame_natural(160 + 8 * i, 120 + 4 * i, 60 + i) for i in range(5)]
    info = str(tmp_path / "set" / "info.dat")
    images, rects = cc.create_test_samples(info, obj, bgs, 5, 24, 24, maxscale=3.0)
    assert len(images) == 5 and len({tuple(r[2:]) for r in rects.tolist()}) > 1
    vec = str(tmp_path / "positives.vec")
    out = cc.create_samples_from_info(vec, info, num=1000, w=24, h=24, max_batch=2)
    want = np.stack([AW.sample(img, r, 24, 24) for img, r in zip(images, rects.tolist())])
    _same(out, want)
    _same(vec_read(vec).reshape(-1, 24, 24), want)
    _same(cc.create_samples_from_info(vec, info, num=3), want[:3])


def _status(images, records, win, n=None, out=True, device=None):
    imgs = [np.ascontiguousarray(i) for i in images]
    recs = np.ascontiguousarray(records, np.int32).reshape(-1, 5)
    ptrs = (C.c_void_p * max(len(imgs), 1))(*[i.ctypes.data for i in imgs])
    ws = np.array([i.shape[1] for i in imgs], np.int32)
    hs = np.array([i.shape[0] for i in imgs], np.int32)
    st = np.array([i.strides[0] for i in imgs], np.uintp)
    buf = np.full((max(len(recs), 1), max(win[1], 1), max(win[0], 1)), 99, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    code = L.lib().cc_samples_from_info(0, C.cast(ptrs, C.c_void_p), vp(ws), vp(hs), vp(st), len(imgs), vp(recs),
                                        len(recs) if n is None else n, win[0], win[1], 0, vp(buf) if out else None, device)
    return code, buf


def test_refusals_and_the_call_after_them():
    images, records, win = info_case("corners")
    want = info_want("corners")

    def works():
        code, buf = _status(images, records, win)
        assert code == L.CC_OK
        _same(buf, want)

    works()
    for label, (field, value) in RECORD_REFUSALS.items():
        bad = [list(r) for r in records]
        bad[1][field] = value
        code, buf = _status(images, bad, win)
        assert code == L.CC_ERR_INVALID_ARG and "record 1:" in L.lib().cc_last_error().decode(), label
        assert (buf == 99).all(), label  # nothing written
        works()
    for bad_win in ((0, 24), (24, 0), (4097, 24), (24, 4097)):
        assert _status(images, records, bad_win)[0] == L.CC_ERR_INVALID_ARG
    works()
    assert _status(images, records, win, n=-1)[0] == L.CC_ERR_INVALID_ARG
    assert _status(images, records, win, out=False)[0] == L.CC_ERR_INVALID_ARG
    assert _status(images + [np.zeros((8193, 2), np.uint8)], records, win)[0] == L.CC_ERR_INVALID_ARG  # an image side of 8193
    w, h = OVERFLOW_SIDES
    code, _ = _status(images + [np.zeros((h, w), np.uint8)], list(records) + [(2, 0, 0, w, h)], (1, 1))
    assert code == L.CC_ERR_INVALID_ARG and "record 6:" in L.lib().cc_last_error().decode()
    with pytest.raises(L.CascadeError) as e:
        cc.resize_area(np.zeros((h, w), np.uint8), 1, 1)
    assert e.value.status == L.CC_ERR_INVALID_ARG and "2^31" in str(e.value)
    with pytest.raises(L.CascadeError) as e:  # INTER_AREA proper does not grow a side
        cc.resize_area(images[0], 65, 48)
    assert e.value.status == L.CC_ERR_INVALID_ARG
    assert _status(images, records, win, n=0, out=False)[0] == L.CC_OK  # no record: nothing to write
    works()
