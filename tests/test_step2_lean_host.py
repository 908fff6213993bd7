"""Host side of the specialised Haar kernel's STEP-2 module in the lean LDS layout (no device): the LDS sum and the
blocks per CU it runs (in allocation units) at 8 to 12 rows for windows of 20x20, 24x24 and 32x32, the height the library picks, the
module's wave_below, and the layout's index arithmetic restated in tests/step2_lean.py -- norm-factor slots, the two queue
tables, the split phase's partial sums for every (rows, slices) the kernel can choose, the wave phase's lists, and the row
ownership of the dense phase. Every check is also shown to fail for the obvious wrong variant (the padded pitch, a gap
that counts bytes the area does not have, lists in the table that is read, whole-rows-per-wavefront ownership): these host mutations stand in for
device ones."""
import ctypes as C

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from tests import haar_windows as hw
from tests import step2_lean as t


def _xml(window):
    W, H = window
    return hw.stump_xml(W, H, False)


def _plan(xml_text, rows_wanted=0, wave_below=24):
    p = cc.CascadeClassifier()
    assert p.load_from_string(xml_text)
    rows, lds, blocks, wb = C.c_int(), C.c_size_t(), C.c_int(), C.c_int()
    st = L.lib().cc_debug_spec_step2_plan(p._c, rows_wanted, wave_below, C.byref(rows), C.byref(lds), C.byref(blocks), C.byref(wb))
    return st, rows.value, lds.value, blocks.value, wb.value


def test_lds_sum_of_the_24x24_window():
    """tile rows of 154 words (skew 20); request, allocation units and blocks per CU per height. 10 rows are
    exactly 25 units; the padded 8-row module this one replaces asked for 31 072 bytes, 25 units as well. A request of a
    fifth of the CU's 160 KiB is 26 units and runs four blocks, whatever 163 840 // 32 768 says."""
    assert t.row_stride_step2(24) == 154 and t.skew_step2(24) == 20
    quoted = {8: (28512, 23, 5), 9: (30256, 24, 5), 10: (32000, 25, 5), 11: (33744, 27, 4), 12: (35488, 28, 4)}
    for rows, (nbytes, units, blocks) in quoted.items():
        assert t.lean_lds_bytes(24, 24, rows) == nbytes and -(-nbytes // t.ALLOC) == units
        assert t.blocks_per_cu(nbytes) == blocks
        assert _plan(_xml((24, 24)), rows)[:4] == (0, rows, nbytes, blocks)
    assert t.padded_lds_bytes(24, 24) == 31072 and t.blocks_per_cu(31072) == 5
    assert [t.blocks_per_cu(n) for n in (32000, 32256, 32512, 32768)] == [5, 4, 4, 4]  # measured: EXPERIMENTS 3.24
    assert [t.blocks_by_bytes(n) for n in (32000, 32256, 32512, 32768)] == [5, 5, 5, 5]
    assert _plan(_xml((24, 24)))[:4] == (0, 10, 32000, 5)


@pytest.mark.parametrize("window", t.WINDOWS, ids=lambda w: "%dx%d" % w)
def test_request_blocks_and_default_height(window):
    """The library's sum is the restated one at every height; the height picked is the tallest with the blocks of 8 rows,
    which are no fewer than the padded 8-row module had (all counted in allocation units)."""
    W, H = window
    xml = _xml(window)
    for rows in t.HEIGHTS:
        nbytes = t.lean_lds_bytes(W, H, rows)
        assert nbytes % 16 == 0 and t.blocks_per_cu(nbytes) <= t.blocks_by_bytes(nbytes)
        assert _plan(xml, rows)[:4] == (0, rows, nbytes, t.blocks_per_cu(nbytes))
    st, rows, lds, blocks, _ = _plan(xml)
    want = t.default_rows(W, H)
    assert (st, rows, lds) == (0, want, t.lean_lds_bytes(W, H, want))
    assert blocks == t.blocks_per_cu(t.lean_lds_bytes(W, H, 8)) >= t.blocks_per_cu(t.padded_lds_bytes(W, H))
    assert want == 12 or t.blocks_per_cu(t.lean_lds_bytes(W, H, want + 1)) < blocks


def test_heights_and_cascades_the_module_does_not_take(lbp_xml):
    xml = _xml((24, 24))
    assert _plan(xml, 7)[0] == L.CC_ERR_INVALID_ARG and _plan(xml, 13)[0] == L.CC_ERR_INVALID_ARG
    assert _plan(open(lbp_xml).read())[0] == L.CC_ERR_UNSUPPORTED
    assert _plan(hw.stump_xml(24, 24, True))[0] == L.CC_ERR_UNSUPPORTED  # tilted features: one module at the library's height


def test_wave_below_of_the_module(monkeypatch):
    xml = _xml((24, 24))
    for k in ("CCAMD_WAVE_BELOW", "CCAMD_WAVE_BELOW1", "CCAMD_WAVE_BELOW2"):
        monkeypatch.delenv(k, raising=False)
    assert [_plan(xml, rows)[4] for rows in t.HEIGHTS] == [24] * 5  # the detector's value (profiles/EXPERIMENTS.md 3.24)
    assert _plan(xml, 10, wave_below=0)[4] == 0  # no wave phase for the cascade: none for the module
    monkeypatch.setenv("CCAMD_WAVE_BELOW1", "40")  # the STEP-1 module's variable is not this module's
    assert _plan(xml, 10)[4] == 24
    monkeypatch.setenv("CCAMD_WAVE_BELOW2", "40")
    assert _plan(xml, 10)[4] == 40
    monkeypatch.setenv("CCAMD_WAVE_BELOW2", "100")
    assert _plan(xml, 10)[4] == 64  # a wavefront's share must fit its 64 lanes


@pytest.mark.parametrize("rows", t.HEIGHTS)
@pytest.mark.parametrize("window", t.WINDOWS, ids=lambda w: "%dx%d" % w)
def test_norm_factor_slots(rows, window):
    """slot = 64 r + ((x + r skew) mod 64) is one to one onto [0, 64 rows) and its bank is the window's bank class."""
    skew = t.skew_step2(window[0])
    assert skew % 8 == 4
    ids = np.arange(rows * 64)
    slot = t.vnf_slot(ids, skew)
    assert sorted(slot.tolist()) == ids.tolist()
    assert ((slot & 31) == t.win_class(ids, skew)).all()
    padded = (ids >> 6) * (64 + skew) + (ids & 63)  # the padded layout's pitch does not fit rows of 64
    assert padded.max() >= rows * 64
    unrotated = ids  # rows of 64 without the rotation: the bank is no longer the class
    assert not ((unrotated & 31) == t.win_class(ids, skew)).all()


@pytest.mark.parametrize("rows", t.HEIGHTS)
def test_queue_area_never_overlaps(rows):
    """While neither table holds more than R rows: the two tables are disjoint and inside the area; the partial sums of every
    slice count the kernel can choose at R rows lie between them, 8-byte aligned; the wave phase's lists lie in the table
    that is not read, beyond anything the table that is read can hold. Slices chosen for a gap that counts 768 bytes the area
    does not have, or a table 1 that starts 768 bytes further back, fail the same checks."""
    entries, qrows = t.queue_entries(rows), 2 * rows
    chosen = {}
    for R in range(0, qrows + 1):
        t0, t1 = t.table_entries(0, R, entries), t.table_entries(1, R, entries)
        assert len(t0 | t1) == 2 * R * 32 and all(0 <= i < entries for i in t0 | t1)
        assert t.gap_bytes(rows, R) == (entries - 2 * R * 32) * 2
        for ns in t.slices_chosen(rows, R):
            chosen.setdefault(ns, []).append(R)
            if ns > 1:
                part = t.split_entries(R, ns)
                assert not part & (t0 | t1) and max(part) < entries and (R * 32 * 2) % 8 == 0
    for g in (0, 1):
        lists = t.wave_list_entries(g, entries)
        assert all(0 <= i < entries for i in lists) and not lists & t.table_entries(g, qrows, entries)
    assert chosen.get(1) and chosen.get(2) and chosen.get(4)  # every split width and the unsplit fallback occur
    # mutation 1: a gap that counts bytes the area does not have
    hit = False
    for R in range(0, qrows + 1):
        for ns in t.slices_chosen(rows, R, extra=768):
            if ns > 1 and t.split_entries(R, ns) & t.table_entries(1, R, entries):
                hit = True
    assert hit
    # mutation 2: table 1 counted back from an end 768 bytes behind the area's: its first rows lie in the counters
    assert any(i >= entries for i in t.table_entries(1, 1, entries + 384))
    # mutation 3: the lists of an even group at the front of the area, where the table it reads begins
    assert t.wave_list_entries(1, entries) & t.table_entries(0, qrows, entries)


def test_slices_at_ten_rows():
    """What fits between the tables of the 10-row tile: four slices (1 536 bytes) up to 8 queued rows, two (1 024) up to 12,
    none beyond; one leftover row group asks for four, two ask for two, three for none."""
    def most(ns):
        return max(R for R in range(21) if t.split_need_bytes(ns) <= t.gap_bytes(10, R))
    assert (most(4), most(2)) == (8, 12)
    assert t.slices_chosen(10, 1) == {4} and t.slices_chosen(10, 9) == {2} and t.slices_chosen(10, 17) == {1}
    assert t.slices_chosen(10, 3) == {2} and t.slices_chosen(10, 11) == {2} and t.slices_chosen(10, 19) == {1}
    assert t.slices_chosen(10, 5) == {1} and t.slices_chosen(10, 8) == set()


@pytest.mark.parametrize("rows", tuple(range(4, 33)))
def test_row_ownership_covers_every_row_once(rows):
    owned = [r for w in range(t.WAVES) for r in t.owned_rows(w, rows)]
    assert sorted(owned) == list(range(rows))
    per = t.rows_per_thread(rows)
    assert all(len(t.owned_rows(w, rows)) in (per, per - 1) for w in range(t.WAVES))
    if rows % t.WAVES:
        # whole rows per wavefront with the rounded-down count loses rows, with the rounded-up count it leaves the tile
        assert t.WAVES * (rows // t.WAVES) < rows
        assert max(w * per + k for w in range(t.WAVES) for k in range(per)) >= rows
        assert [len(t.owned_rows(w, rows)) for w in range(t.WAVES)] == [per] * (rows % t.WAVES) + [per - 1] * (t.WAVES - rows % t.WAVES)


def test_frames_of_the_gpu_test_give_their_grids():
    sizes = t.edge_frame_sizes()
    grids = {t.grid_at_scale_1(w, h) for (w, h) in sizes}
    assert {(nx, ny) for nx in t.NX_TARGETS for ny in t.NY_TARGETS} <= grids
    assert {(w, h) for w in t.FRAME_WIDTHS for h in t.FRAME_HEIGHTS} <= set(sizes)
    assert max(w for w, _ in sizes) == 152 and max(h for _, h in sizes) == 65 and len(sizes) <= 56
    assert [t.grid_at_scale_1(w, 24)[0] for w in t.FRAME_WIDTHS] == list(t.NX_TARGETS)
