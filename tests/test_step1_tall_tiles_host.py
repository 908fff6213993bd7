"""Host side of the specialised Haar kernel's STEP-1 module (no device): the LDS request of its lean layout per tile height,
the blocks per CU DESIGN.md 4.4 quotes for it, the height the library picks for a window, the module's wave_below, the
layout's own index arithmetic (restated: norm-factor slots, queue tables, what lives between them) and the frame shapes
tests/test_gpu_step1_tall_tiles.py runs."""
import ctypes as C

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from tests import haar_windows as hw
from tests import step1_tall as t


def _plan(xml_text, rows_wanted=0, wave_below=24):
    p = cc.CascadeClassifier()
    assert p.load_from_string(xml_text)
    rows, lds, blocks, wb = C.c_int(), C.c_size_t(), C.c_int(), C.c_int()
    st = L.lib().cc_debug_spec_step1_plan(p._c, rows_wanted, wave_below, C.byref(rows), C.byref(lds), C.byref(blocks), C.byref(wb))
    return st, rows.value, lds.value, blocks.value, wb.value


def test_lds_request_and_blocks_per_cu_of_the_24x24_window():
    """The figures of DESIGN.md 4.4: bytes per block and blocks per CU at 12, 16, 20 and 24 rows (before the lean layout:
    22 272, 26 240, 30 208 and 34 176 bytes = 7, 6, 5 and 4 blocks)."""
    xml = hw.stump_xml(24, 24, False)
    quoted = {12: (19200, 8), 16: (22656, 7), 20: (26112, 6), 24: (29568, 5)}
    for rows, (nbytes, blocks) in quoted.items():
        assert t.lean_lds_bytes(24, 24, rows) == nbytes and t.blocks_per_cu(nbytes) == blocks
        st, r, lds, b, _ = _plan(xml, rows)
        assert (st, r, lds, b) == (0, rows, nbytes, blocks)
    old = {rows: t.lean_lds_bytes(24, 24, rows) + 3 * 64 * 8 + rows * 32 * 4 for rows in quoted}  # + s_part + the vnf rows' padding
    assert old == {12: 22272, 16: 26240, 20: 30208, 24: 34176}
    assert [t.blocks_per_cu(v) for v in old.values()] == [7, 6, 5, 4]


@pytest.mark.parametrize("window", [(24, 24)] + hw.WINDOWS, ids=lambda w: "%dx%d" % w)
def test_request_and_default_height_of_every_window(window):
    """Every window size of tests/haar_windows.py: the request at each height is the restated one, and the library's own
    choice is its default height (20 rows) or, where that leaves fewer than four blocks per CU, the tallest height below
    it that does not, and 8 rows where none does."""
    W, H = window
    xml = hw.stump_xml(W, H, False)
    for rows in (8,) + t.HEIGHTS + (32,):
        st, r, lds, b, _ = _plan(xml, rows)
        assert (st, r, lds, b) == (0, rows, t.lean_lds_bytes(W, H, rows), t.blocks_per_cu(t.lean_lds_bytes(W, H, rows)))
    st, r, lds, b, _ = _plan(xml)
    want = t.default_rows(W, H, 20)
    assert (st, r, lds) == (0, want, t.lean_lds_bytes(W, H, want))
    assert b >= 4 or want == 8
    if want < 20:
        assert t.blocks_per_cu(t.lean_lds_bytes(W, H, want + 4)) < 4
    if window in ((24, 24), (20, 20), (25, 24)):
        assert r == 20


def test_wave_below_of_the_module():
    xml = hw.stump_xml(24, 24, False)
    assert [_plan(xml, rows)[4] for rows in (8, 12, 16, 20, 24)] == [24, 32, 32, 32, 32]
    assert _plan(xml, 20, wave_below=0)[4] == 0  # no wave phase for the cascade: none for the module
    assert _plan(xml, 20, wave_below=48)[4] == 48


def test_cascades_without_such_a_module(lbp_xml):
    assert _plan(open(lbp_xml).read())[0] == L.CC_ERR_UNSUPPORTED
    assert _plan(hw.stump_xml(24, 24, True))[0] == L.CC_ERR_UNSUPPORTED  # tilted features: one module at the library's height
    assert _plan(hw.stump_xml(24, 24, False), 18)[0] == L.CC_ERR_INVALID_ARG  # not a whole number of rows per wavefront


@pytest.mark.parametrize("rows", t.HEIGHTS + (8, 28, 32))
@pytest.mark.parametrize("window", [(24, 24), (20, 20), (25, 24), (19, 23)], ids=lambda w: "%dx%d" % w)
def test_lean_layout_indices(rows, window):
    """The layout's arithmetic, restated. Norm factors: slot = 64 r + ((x + r skew) mod 64) is one to one onto [0, 64 rows),
    and its bank (slot mod 32) is the window's bank class (x + r skew) mod 32. Queue tables of `2 rows` rows of 32 entries:
    table 0 from the front, table 1 from the back; while neither holds more than R rows, the entries between them are
    untouched, and the split phase is allowed as many slices as fit there; the wave phase's four lists of 64 ids lie in the
    table that is not read, beyond anything the table that is read can hold."""
    W, H = window
    stride = t.tile_words_step1(W, H, rows) // ((rows - 1) + H + 1)
    skew = stride & 31
    assert skew % 16 != 0
    ids = np.arange(rows * 64)
    r, x = ids >> 6, ids & 63
    slot = (ids & ~63) | ((x + skew * r) & 63)
    assert sorted(slot.tolist()) == ids.tolist()
    padded = r * (64 + skew) + x  # the padded layout's slot does not fit rows of 64: this is what the rotation replaces
    assert padded.max() >= rows * 64 and len(set(padded.tolist())) == len(ids)
    assert ((slot & 31) == ((x + skew * r) & 31)).all()
    qrows, entries = 2 * rows, 2 * rows * 64

    def q_index(g, row, c):
        return (2 * qrows - 1 - row) * 32 + c if g & 1 else row * 32 + c
    for R in range(0, qrows + 1):
        used = {q_index(g, row, c) for g in (0, 1) for row in range(R) for c in range(32)}
        assert len(used) == 2 * R * 32 and all(0 <= i < entries for i in used)
        gap_lo, gap_bytes = R * 32, entries * 2 - 2 * R * 64
        assert all(not (gap_lo <= i < gap_lo + gap_bytes // 2) for i in used)
        for ns in (2, 4):  # slices 1 .. ns-1, 256 / ns doubles each
            need = (ns - 1) * (256 // ns) * 8
            if need <= gap_bytes:
                assert gap_lo * 2 % 8 == 0 and gap_lo * 2 + need <= entries * 2 - R * 64
    for g in (0, 1):
        lists = range(0, 256) if g & 1 else range(entries - 256, entries)
        read = {q_index(g, row, c) for row in range(qrows) for c in range(32)}
        assert not read & set(lists)


@pytest.mark.parametrize("rows", t.HEIGHTS)
def test_edge_frames_cover_their_targets(rows):
    for (W, H) in ((24, 24), (20, 20), (25, 24)):
        frames = t.edge_frames(W, H, rows)
        assert len(frames) <= 5 and all(150 <= w <= 220 and 90 <= h <= 160 for w, h in frames)
        assert t.covered_targets(W, H, rows, frames) == set(t.ny_targets(rows)) | set(t.nx_targets())
