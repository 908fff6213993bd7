"""The Haar wave phase with integer vote sums against the CPU oracle, bit for bit: result codes, stage sums (compared as
uint64), visited flags and the rectangles of detect_batch, for the table-driven and the run-time specialised kernel, with
the integer form on and off (CCAMD_WAVE_INT) and wavefront shares of at most 6 and at most 16 windows (CCAMD_WAVE_BELOW 24 /
64).

Cascades (tests/wave_int_cases.py; tests/test_wave_int_host.py shows what their tables are): the headline cascade, whose
stages up to 10 have the integer form and 11-24 do not, so one launch runs both; b_below / b_at on either side of the int32
bound; 'chunks' with late stages of 63, 64, 65, 128 and 129 stumps, the 64-stump stage with a threshold that windows hit
exactly (a tie passes: the test is !(sum < threshold)).

Every case first shows, from the oracle's codes and wave_below alone, that windows are rejected by and pass stages with
the integer form while their tile is in the wave phase."""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from oracle import oracle as orc
from tests import cascade_edges as ce
from tests import wave_int_cases as wi

pytestmark = pytest.mark.gpu

NAMES = ["headline", "b_below", "b_at", "chunks"]
SPEC_STAGES = {"headline": 7, "b_below": 2, "b_at": 2, "chunks": 2}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("wave_int")


@pytest.fixture(scope="module")
def refs(tmp):
    """name -> (oracle cascade, integer-form flags per stage, [(oracle result, grouped rectangles) per frame]); shared, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            o = wi.oracle_cascade(tmp, name)
            form = [q is not None for q in wi.expected_tables(o)[0]]
            res = []
            for img in wi.frames():
                ref = orc.detect_raw(o, img, wi.SCALE_FACTOR, nthreads=8, full=True)
                res.append((ref, orc.group_rectangles(ref.candidates[:, 3:7], 2, 0.2)))
            cache[name] = (o, form, res)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def chunk_ties(refs):
    """Per frame, the windows of 'chunks' whose sum at the tie stage equals its threshold: those that the oracle passes
    through the cascade cut after that stage with exactly that sum. Computed once, on first use."""
    cache = []

    def get():
        if not cache:
            o, _, _ = refs("chunks")
            cut = ce.truncated(o, wi.CHUNK_TIE_STAGE)
            t = np.float64(ce.effective_threshold(o.stage_threshold[wi.CHUNK_TIE_STAGE]))
            for img in wi.frames():
                r = orc.detect_raw(cut, img, wi.SCALE_FACTOR, nthreads=8, full=True)
                cache.append((r.codes == 1) & (r.sums == t))
        return cache
    return get


@pytest.mark.parametrize("wave_below", [24, 64])
@pytest.mark.parametrize("wave_int", [0, 1])
@pytest.mark.parametrize("spec", [False, True], ids=["tables", "specialised"])
@pytest.mark.parametrize("name", NAMES)
def test_wave_phase_integer_sums(refs, chunk_ties, name, spec, wave_int, wave_below, monkeypatch):
    o, form, res = refs(name)
    # the condition: the oracle alone shows both outcomes in integer-form stages of the wave phase, on each frame
    for img, (ref, _) in zip(wi.frames(), res):
        rej, pas = wi.wave_phase_windows(o, img, ref.codes, wave_below, form)
        assert rej.any() and pas.any(), f"{name}: {int(rej.sum())} rejected, {int(pas.sum())} passed"
    if name == "chunks":  # the tie: windows of the wave phase whose sum IS the tie stage's threshold, and they go on
        n_ties = 0
        for img, (ref, _), tie in zip(wi.frames(), res, chunk_ties()):
            _, went_on = wi.wave_phase_windows(o, img, ref.codes, wave_below, [s == wi.CHUNK_TIE_STAGE for s in range(o.nstages)])
            n_ties += int((went_on & tie).sum())
        assert n_ties > 0
    monkeypatch.setenv("CCAMD_WAVE_INT", str(wave_int))
    monkeypatch.setenv("CCAMD_WAVE_BELOW", str(wave_below))
    p = cc.CascadeClassifier(max_batch=2)
    assert p.load_from_string(wi.xml_text(name)), getattr(p, "load_error", "")
    if spec:
        assert p.specialize(SPEC_STAGES[name]) == SPEC_STAGES[name]
    n = 0
    for img, (ref, _) in zip(wi.frames(), res):
        codes, sums, vis = p.debug_windows(img, wi.SCALE_FACTOR)
        assert len(codes) == ref.n_grid_windows
        bad = np.nonzero(codes != ref.codes)[0]
        assert len(bad) == 0, f"{len(bad)} of {len(codes)} window results differ, first at {bad[:5].tolist()}: {codes[bad[:5]].tolist()} for {ref.codes[bad[:5]].tolist()}"
        bad = np.nonzero(sums.view(np.uint64) != ref.sums.view(np.uint64))[0]
        assert len(bad) == 0, f"{len(bad)} stage sums differ, first {sums[bad[:3]].tolist()} for {ref.sums[bad[:3]].tolist()} (codes {codes[bad[:3]].tolist()})"
        assert (vis == ref.visited).all()
        n += len(ref.candidates)
    assert n > 0
    got = p.detect_batch(np.stack(wi.frames()), wi.SCALE_FACTOR, 2)
    assert len(got) == 2
    for g, (_, grouped) in zip(got, res):
        assert g.shape == grouped.shape and (g == grouped).all()
