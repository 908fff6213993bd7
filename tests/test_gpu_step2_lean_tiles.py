"""The run-time specialised Haar kernel's STEP-2 module in the lean LDS layout, at tile heights that are no multiple of the
block's wavefronts: every window's result code, exit stage, stage sum (tolerance 0), visited flag and every rectangle equal
the CPU oracle's.

Heights 8 to 12 are forced with CCAMD_SPEC_TILE_Y2 (read when a module is built). Frames of 24..152 x 24..65 pixels give the
largest STEP-2 scale 1, 9, 10, 11, 19, 20 and 21 window rows and 1, 63, 64 and 65 window columns (tests/step2_lean.py;
checked on the host by tests/test_step2_lean_host.py), one frame of 280x90 has levels of several tiles both ways. A cascade
whose first four stages pass every window fills both queue tables while the gap between them is smallest and then thins the
tile through every row count. Cascades whose modules the change does not touch (other windows at their own height, tilted,
LBP) are compared with the oracle as well."""
import functools
import re

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from oracle import oracle as orc
from tests import haar_windows as hw
from tests import step2_lean as t
from tests.step1_tall import same_as_oracle
from tests.util import frame_natural

pytestmark = pytest.mark.gpu

_ENV = ("CCAMD_SPEC_TILE_Y", "CCAMD_SPEC_TILE_Y1", "CCAMD_SPEC_TILE_Y2", "CCAMD_SPEC_ONE_MODULE", "CCAMD_WAVE_BELOW", "CCAMD_WAVE_BELOW1",
        "CCAMD_WAVE_BELOW2", "CCAMD_SPLIT_STUMPS")


@pytest.fixture
def clean_env(monkeypatch):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _classifier(text, k):
    p = cc.CascadeClassifier()
    assert p.load_from_string(text)
    assert p.specialize(k) == k
    return p


_TRACE = re.compile(r"tiles of step (\d) \(0 = all\), (\d+) window rows, (\d+) bytes of LDS per block, (\d+) resident blocks per CU, (-?\d+) bytes of scratch")


def _traced_classifier(text, k, monkeypatch, capfd):
    """The classifier and what the library says it loaded: {step: (rows, LDS bytes, blocks per CU by the runtime's occupancy
    query, scratch bytes per lane)} from the CCAMD_TRACE_HOST lines of this specialisation."""
    monkeypatch.setenv("CCAMD_TRACE_HOST", "1")
    capfd.readouterr()
    p = _classifier(text, k)
    err = capfd.readouterr().err
    monkeypatch.delenv("CCAMD_TRACE_HOST")
    return p, {int(m[0]): tuple(int(v) for v in m[1:]) for m in _TRACE.findall(err)}


@functools.lru_cache(maxsize=None)
def _edge_frames():
    """One frame per size of tests/step2_lean.py's edge_frame_sizes, calibration windows pasted at the largest scales where they fit."""
    frames = [hw.pasted_frame(24, 24, 100 + i, w=w, h=h, scales=(1.0, 1.3)) for i, (w, h) in enumerate(t.edge_frame_sizes())]
    frames.append(hw.pasted_frame(24, 24, 140, w=280, h=90, scales=(1.0, 1.3, 1.7)))
    return frames


@functools.lru_cache(maxsize=None)
def _edge_cascade(tmp):
    text = hw.stump_xml(24, 24, False)
    return text, hw.oracle_cascade(tmp, text, "c24.xml")


@pytest.mark.parametrize("rows", t.HEIGHTS)
def test_tile_edges_at_every_height(rows, clean_env, capfd, tmp_path_factory):
    text, o = _edge_cascade(str(tmp_path_factory.getbasetemp()))
    clean_env.setenv("CCAMD_SPEC_TILE_Y2", str(rows))
    p, built = _traced_classifier(text, 4, clean_env, capfd)
    # the module really has the forced height, the restated request, no scratch, and the occupancy query's answer
    # (which counts bytes, not allocation units: 5 blocks at every height up to 10, 4 beyond)
    assert built[2] == (rows, t.lean_lds_bytes(24, 24, rows), t.blocks_by_bytes(t.lean_lds_bytes(24, 24, rows)), 0), built
    assert built[1][0] == 20  # the STEP-1 module beside it keeps its height
    n = 0
    for img in _edge_frames():
        n += same_as_oracle(p, o, img)
    assert n > 0
    # two stages compiled: the table-driven stages (split by stumps, wave phase) read the same layout
    p = _classifier(text, 2)
    for img in _edge_frames()[-5:]:
        same_as_oracle(p, o, img)


@functools.lru_cache(maxsize=None)
def _capacity_case(tmp):
    text = t.pass_all_then_thin_xml(hw.calibration_windows(24, 24))
    o = hw.oracle_cascade(tmp, text, "thin.xml")
    # textured everywhere (no window fails the variance test), 3 x 3 tiles of 10 rows at scale 1
    img = frame_natural(320, 80, 31)
    wins = hw.calibration_windows(24, 24)
    rng = np.random.default_rng(7)
    for k in range(40):  # windows the thinning stages were calibrated on: queues that stay long
        x, y = int(rng.integers(0, 320 - 24)), int(rng.integers(0, 80 - 24))
        img[y:y + 24, x:x + 24] = wins[int(rng.integers(0, len(wins)))]
    ref = orc.detect_raw(o, img, t.SCALE_FACTOR, nthreads=8, full=True)
    return text, o, img, ref


@pytest.mark.timeout(120)
@pytest.mark.parametrize("wave_below", [0, 24, 40])
@pytest.mark.parametrize("rows", [9, 10, 11])
def test_full_queue_tables_then_every_row_count(rows, wave_below, clean_env, tmp_path_factory):
    """Modelled on test_every_late_stage_shape_in_one_launch. The first four stages pass every window: both queue tables
    hold all 64 x rows ids, the gap between them is at its smallest and stage after stage runs unsplit. The stages behind
    them keep about 80 % each, so the tiles walk down through every row count: split by four, by two where four no longer
    fit the gap, unsplit where two do not, and (wave_below > 0) the wave phase -- all in the launches of one frame. The
    oracle's codes say so before the device is asked."""
    text, o, img, ref = _capacity_case(str(tmp_path_factory.getbasetemp()))
    sc = cc.scale_plan(24, 24, img.shape[1], img.shape[0], t.SCALE_FACTOR)
    nx, ny = int(sc[0]["nx"]), int(sc[0]["ny"])
    assert int(sc[0]["ystep"]) == 2 and nx > 2 * 64 and ny > 2 * rows
    codes0 = ref.codes[:nx * ny]
    n_stages = 20
    full = (codes0.reshape(ny, nx)[:rows, :64] <= -4) | (codes0.reshape(ny, nx)[:rows, :64] == 1)
    assert full.all()  # the first tile enters stage 4 with all its windows: 2 x rows rows in both tables
    seen = set()
    per_stage = t.late_rows_per_tile(codes0, nx, ny, rows, t.skew_step2(24), n_stages)
    for s in range(4, n_stages):
        seen |= per_stage[s]
    widths = set()
    for R in seen:
        widths |= t.slices_chosen(rows, R)
    assert {1, 2, 4} <= widths, (sorted(seen), widths)
    assert 2 * rows in seen and len(seen) > rows  # from full tables down through most row counts
    fallback = [R for R in seen if t.slices_chosen(rows, R) != t.slices_chosen(rows, R, extra=1 << 20)]
    assert fallback  # some tile asks for more slices than fit the gap
    counts = set()
    for s, c in t.late_counts_per_tile(codes0, nx, ny, rows, n_stages).items():
        if s >= 4:
            counts |= c
    if wave_below:  # some tiles enter a stage with fewer windows than wave_below (wave phase), others with more (thread phase)
        assert any(0 < n < wave_below for n in counts) and any(n >= wave_below for n in counts), sorted(counts)
    clean_env.setenv("CCAMD_SPEC_TILE_Y2", str(rows))
    clean_env.setenv("CCAMD_WAVE_BELOW2", str(wave_below))
    for k in (20, 4):  # every stage compiled; the thinning stages table-driven
        p = _classifier(text, k)
        assert same_as_oracle(p, o, img) >= 0


@pytest.mark.parametrize("window", [(20, 20), (32, 32)], ids=lambda w: "%dx%d" % w)
def test_other_windows_at_their_own_height(window, clean_env, capfd, tmp_path):
    W, H = window
    text = hw.stump_xml(W, H, False)
    o = hw.oracle_cascade(tmp_path, text)
    p, built = _traced_classifier(text, 4, clean_env, capfd)
    rows = t.default_rows(W, H)
    assert built[2][:2] == (rows, t.lean_lds_bytes(W, H, rows)), built
    n = 0
    for i, (w, h) in enumerate(((2 * 64 + W + 3, 2 * rows + H + 1), (2 * 63 + W - 1, 2 * (rows + 1) + H - 1), (300, 120))):
        n += same_as_oracle(p, o, hw.pasted_frame(W, H, 50 + i, w=w, h=h, scales=(1.0, 1.3, 2.3)))
    assert n > 0


def test_tilted_and_lbp_modules_are_untouched(lbp_xml, clean_env, tmp_path):
    text = hw.stump_xml(24, 24, True)
    o = hw.oracle_cascade(tmp_path, text)
    p = _classifier(text, 4)
    n = same_as_oracle(p, o, hw.pasted_frame(24, 24, 60, w=300, h=120, scales=(1.0, 1.3, 2.3)))
    q = cc.CascadeClassifier(lbp_xml)
    assert q.specialize(20) == 20
    n += same_as_oracle(q, orc.load_cascade_xml(lbp_xml), frame_natural(320, 200, 61))
    assert n > 0


def test_default_module_of_the_24x24_window(clean_env, capfd, tmp_path_factory):
    """Nothing forced: 10 rows, 32 000 bytes, 5 blocks per CU by hipModuleOccupancyMaxActiveBlocksPerMultiprocessor, no
    scratch. A height outside 8..12 is ignored and gives the same module."""
    text, _ = _edge_cascade(str(tmp_path_factory.getbasetemp()))
    _, built = _traced_classifier(text, 4, clean_env, capfd)
    assert built[2] == (10, 32000, 5, 0), built
    clean_env.setenv("CCAMD_SPEC_TILE_Y2", "16")
    _, built = _traced_classifier(text, 4, clean_env, capfd)
    assert built[2] == (10, 32000, 5, 0), built
