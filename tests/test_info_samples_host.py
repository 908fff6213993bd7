"""The host side of the -info mode without a device: the fscanf walk over an info file (scan_info), what
create_samples_from_info does around the device call (the device call itself replaced by the witness), the command line,
the bindings, and the refusals cc_samples_from_info makes before it touches a device."""
import ctypes as C
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import samples as S
from cascadeclassifier_amd.detector import resize_area, vec_read
from tests import area_witness as AW
from tests.info_cases import OVERFLOW_SIDES, RECORD_REFUSALS, info_case, random_image


@pytest.fixture
def on_witness(monkeypatch):
    """create_samples_from_info with the witness in the place of the device: everything else is the product's."""
    calls = []

    def stand_in(images, records, win, device=0, max_batch=0, device_out=None, host=True):
        recs = [tuple(r) for r in np.asarray(records).reshape(-1, 5).tolist()]
        calls.append((len(images), recs))
        return AW.samples(images, recs, win[0], win[1])

    monkeypatch.setattr(S, "samples_from_info", stand_in)
    return calls


def _files(tmp_path, text, images):
    for name, img in images.items():
        if name.endswith(".npy"):
            np.save(str(tmp_path / name), img)
        else:
            S.write_gray(str(tmp_path / name), img)
    (tmp_path / "info.dat").write_text(text)
    return str(tmp_path / "info.dat")


def test_tokens_may_be_split_anyhow(tmp_path):
    info = _files(tmp_path, "a.pgm\n2\t1 2\n3 4   5\r\n6 7 8\n\n\nb.npy 1\n0 0 9 9", {})
    entries, bad = S.scan_info(info, 1000)
    assert bad is None and entries == [("a.pgm", [(1, 2, 3, 4), (5, 6, 7, 8)]), ("b.npy", [(0, 0, 9, 9)])]
    S.write_info(info, entries)  # what write_info writes is read back
    assert S.scan_info(info, 1000) == (entries, None)
    assert [(n, r.tolist()) for n, r in S.read_info(info)] == [(n, [list(x) for x in r]) for n, r in entries]


def test_count_of_zero_and_num_cut(tmp_path):
    info = _files(tmp_path, "none.pgm 0\na.pgm 3 1 1 2 2 3 3 4 4 5 5 6 6\nb.pgm 2 0 0 1 1 2 2 3 3\n", {})
    assert S.scan_info(info, 1000) == ([("none.pgm", []), ("a.pgm", [(1, 1, 2, 2), (3, 3, 4, 4), (5, 5, 6, 6)]),
                                        ("b.pgm", [(0, 0, 1, 1), (2, 2, 3, 3)])], None)
    assert S.scan_info(info, 2) == ([("none.pgm", []), ("a.pgm", [(1, 1, 2, 2), (3, 3, 4, 4)])], None)  # cut inside an entry
    assert S.scan_info(info, 3)[0][-1][0] == "a.pgm" and S.scan_info(info, 4)[0][-1] == ("b.pgm", [(0, 0, 1, 1)])
    assert S.scan_info(info, 0) == ([], None)


def test_fscanf_details(tmp_path):
    # "%d" takes the digits from the front of a token and leaves the rest; a name without a count has no rectangles
    info = _files(tmp_path, "a.pgm 1 1 2 3 4x b.pgm 1 5 6 7 8", {})
    # ("4x" gives 4, then "x b.pgm" is a name with no count, then "b.pgm 1 ..." is read as the tool would read it)
    assert S.scan_info(info, 10) == ([("a.pgm", [(1, 2, 3, 4)]), ("x", []), ("b.pgm", [(5, 6, 7, 8)])], None)
    info = _files(tmp_path, "a.pgm 1 -1 +2 3 4", {})
    assert S.scan_info(info, 10) == ([("a.pgm", [(-1, 2, 3, 4)])], None)


def test_fewer_rectangles_than_num_ends_the_run(tmp_path, on_witness):
    img = random_image(64, 48, 21)
    info = _files(tmp_path, "a.pgm 2 0 0 30 26 34 22 30 26\n", {"a.pgm": img})
    vec = str(tmp_path / "deeper" / "out.vec")  # the directory is made, as icvMkDir does
    out = S.create_samples_from_info(vec, info, num=1000)  # the tool would spin here for ever
    assert out.shape == (2, 24, 24) and (out == AW.samples([img], [(0, 0, 0, 30, 26), (0, 34, 22, 30, 26)], 24, 24)).all()
    assert np.frombuffer(open(vec, "rb").read(8), np.int32).tolist() == [2, 24 * 24]  # the header holds the true count
    assert (vec_read(vec) == out.reshape(2, -1)).all()


def test_num_cuts_and_one_image_is_read_once(tmp_path, on_witness):
    a, b = random_image(64, 48, 22), random_image(40, 40, 23)
    text = "a.pgm 2 0 0 30 26 1 1 47 47\nb.npy 1 3 3 20 30\na.pgm 2 5 5 24 24 0 0 64 48\n"
    info = _files(tmp_path, text, {"a.pgm": a, "b.npy": b})
    out = S.create_samples_from_info(str(tmp_path / "o.vec"), info, num=4, w=24, h=24)
    want = [(0, 0, 0, 30, 26), (0, 1, 1, 47, 47), (1, 3, 3, 20, 30), (0, 5, 5, 24, 24)]
    assert on_witness == [(2, want)]  # two images for three entries, four records
    assert (out == AW.samples([a, b], want, 24, 24)).all()
    assert np.frombuffer(open(str(tmp_path / "o.vec"), "rb").read(8), np.int32).tolist() == [4, 576]


def test_malformed_entry_keeps_what_precedes(tmp_path, on_witness, capsys):
    a = random_image(64, 48, 24)
    info = _files(tmp_path, "a.pgm 1 0 0 30 26\na.pgm 2 1 1 25 25 7 seven 30 26\na.pgm 1 0 0 64 48\n", {"a.pgm": a})
    out = S.create_samples_from_info(str(tmp_path / "o.vec"), info, num=10)
    assert capsys.readouterr().err == f"{info}(2) : parse error"
    assert (out == AW.samples([a], [(0, 0, 0, 30, 26), (0, 1, 1, 25, 25)], 24, 24)).all()
    assert len(vec_read(str(tmp_path / "o.vec"))) == 2
    # the file ending inside an entry is the same error, as fscanf returns EOF there
    info = _files(tmp_path, "a.pgm 1 0 0 30 26\na.pgm 2 1 1 25 25 7 7\n", {})
    assert S.scan_info(info, 10) == ([("a.pgm", [(0, 0, 30, 26)]), ("a.pgm", [(1, 1, 25, 25)])], 2)
    out = S.create_samples_from_info(str(tmp_path / "p.vec"), info, num=10)
    assert capsys.readouterr().err == f"{info}(2) : parse error" and len(out) == 2


def test_missing_image_raises_naming_the_file(tmp_path, on_witness):
    a = random_image(64, 48, 25)
    info = _files(tmp_path, "a.pgm 1 0 0 30 26\ngone.pgm 1 0 0 5 5\n", {"a.pgm": a})
    with pytest.raises(ValueError) as e:
        S.create_samples_from_info(str(tmp_path / "o.vec"), info)
    assert "gone.pgm" in str(e.value) and not os.path.exists(str(tmp_path / "o.vec")) and on_witness == []
    (tmp_path / "gone.pgm").write_bytes(b"P6\n1 1\n255\n\0\0\0")  # there, but not a gray image
    with pytest.raises(ValueError) as e:
        S.create_samples_from_info(str(tmp_path / "o.vec"), info)
    assert "gone.pgm" in str(e.value)
    info = _files(tmp_path, "a.pgm 1 0 0 30 26\ngone.pgm 0\nabsent.pgm 0\n", {})  # an image without rectangles is not read
    assert len(S.create_samples_from_info(str(tmp_path / "o.vec"), info)) == 1


def test_barcode_info_fixture_parses(repo_root):
    path = os.path.join(repo_root, "tests", "golden", "barcode.info")
    assert S.scan_info(path, 1000) == ([("ean13_5012345678900.png", [(0, 0, 600, 280)])], None)


def test_command_line_modes_in_the_tools_order():
    assert S.parse_args(["-img", "o.pgm", "-vec", "out.vec"])[0] == "training"
    assert S.parse_args(["-img", "o.pgm", "-vec", "out.vec", "-info", "i.dat", "-bg", "bg.txt"])[0] == "training"
    assert S.parse_args(["-img", "o.pgm", "-vec", "out.vec", "-info", "i.dat"])[0] == "training"
    assert S.parse_args(["-img", "o.pgm", "-bg", "bg.txt", "-info", "i.dat"])[0] == "test"
    mode, a = S.parse_args(["-info", "i.dat", "-vec", "out.vec", "-w", "75", "-h", "32", "-num", "1"])
    assert mode == "from_info" and (a.info, a.vec, a.w, a.h, a.num, a.img) == ("i.dat", "out.vec", 75, 32, 1, None)
    assert S.parse_args(["-info", "i.dat", "-vec", "out.vec", "-bg", "bg.txt"])[0] == "from_info"
    assert S.parse_args(["-info", "i.dat", "-vec", "out.vec"])[1].num == 1000  # the tool's default
    for argv in (["-img", "o.pgm"], ["-img", "o.pgm", "-info", "i.dat"], ["-img", "o.pgm", "-bg", "bg.txt"], ["-vec", "out.vec"],
                 ["-info", "i.dat"], ["-info", "i.dat", "-bg", "bg.txt"], []):
        with pytest.raises(SystemExit):
            S.parse_args(argv)


def test_command_line_runs_the_mode(tmp_path, on_witness, capsys):
    img = random_image(64, 48, 26)
    info = _files(tmp_path, "a.pgm 1 0 0 64 48\n", {"a.pgm": img})
    vec = str(tmp_path / "out.vec")
    assert S.main(["-info", info, "-vec", vec, "-w", "20", "-h", "13", "-num", "5"]) == 0
    assert (vec_read(vec).reshape(1, 13, 20) == AW.samples([img], [(0, 0, 0, 64, 48)], 20, 13)).all()
    assert "1 samples of 20 x 13" in capsys.readouterr().out


def test_symbols_bind_with_declared_argtypes():
    lib = L.lib()
    for name in ("cc_area_tab", "cc_samples_from_info", "cc_samples_from_info_last_ms", "cc_resize_area_u8"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES[name][0], L.SIGNATURES[name][1])
    assert C.sizeof(L.InfoRecord) == 20
    assert cc.create_samples_from_info is S.create_samples_from_info and cc.resize_area is resize_area


def _status(images, records, win, n=None, out=True):
    imgs = [np.ascontiguousarray(i) for i in images]
    recs = np.ascontiguousarray(records, np.int32).reshape(-1, 5)
    ptrs = (C.c_void_p * max(len(imgs), 1))(*[i.ctypes.data for i in imgs])
    ws = np.array([i.shape[1] for i in imgs], np.int32)
    hs = np.array([i.shape[0] for i in imgs], np.int32)
    st = np.array([i.strides[0] for i in imgs], np.uintp)
    buf = np.zeros((max(len(recs), 1), max(win[1], 1), max(win[0], 1)), np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    code = L.lib().cc_samples_from_info(0, C.cast(ptrs, C.c_void_p), vp(ws), vp(hs), vp(st), len(imgs), vp(recs),
                                        len(recs) if n is None else n, win[0], win[1], 0, vp(buf) if out else None, None)
    return code, L.lib().cc_last_error().decode()


def test_refusals_come_before_the_device():
    """Every refusal is CC_ERR_INVALID_ARG whether or not a device is there, and a bad record is named."""
    images, records, win = info_case("corners")
    records = list(records[:3])
    for label, (field, value) in RECORD_REFUSALS.items():
        bad = [list(r) for r in records]
        bad[1][field] = value
        code, msg = _status(images, bad, win)
        assert code == L.CC_ERR_INVALID_ARG and "record 1:" in msg, (label, msg)
    for bad_win in ((0, 24), (24, 0), (4097, 24), (24, 4097), (-1, -1)):
        assert _status(images, records, bad_win)[0] == L.CC_ERR_INVALID_ARG
    assert _status(images, records, win, n=-1)[0] == L.CC_ERR_INVALID_ARG
    assert _status(images, records, win, out=False)[0] == L.CC_ERR_INVALID_ARG  # no output at all
    wide = np.zeros((1, 8193), np.uint8)
    code, msg = _status([images[0], wide], records, win)
    assert code == L.CC_ERR_INVALID_ARG and "image 1:" in msg
    w, h = OVERFLOW_SIDES
    code, msg = _status([images[0], np.zeros((h, w), np.uint8)], records[:1] + [(1, 0, 0, w, h)], (1, 1))
    assert code == L.CC_ERR_INVALID_ARG and "record 1:" in msg and "2^31" in msg
    img = random_image(30, 20, 27)
    dst = np.zeros((24, 24), np.uint8)
    for dw, dh in ((31, 20), (30, 21), (0, 5), (5, 0)):  # INTER_AREA proper shrinks or keeps
        assert L.lib().cc_resize_area_u8(0, img.ctypes.data_as(C.c_void_p), 30, 20, 30, dst.ctypes.data_as(C.c_void_p), dw,
                                         dh) == L.CC_ERR_INVALID_ARG
