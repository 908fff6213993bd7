"""The cascade kernels at the edges of their exactness proofs and shape limits (tests/cascade_edges.py; what each cascade is
and that the oracle alone finds the ties, shares and tile counts on it: tests/test_cascade_edges_host.py).

No tolerance anywhere: per-window result codes, float64 stage sums, visited flags, ungrouped candidates and grouped
rectangles of the table-driven and the run-time specialised detector equal the CPU oracle's, the specialised batch result
equals the table-driven one, and the pass flags of NegativeMiner.run and predict_cascade equal the oracle's reader loop
and stage walk."""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from oracle import oracle as orc
from tests import cascade_edges as ce

pytestmark = pytest.mark.gpu

SPEC_BUDGET = 320  # stumps the specialiser compiles at most (whole stages; cc_spec.hip)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("cascade_edges")


@pytest.fixture(scope="module")
def refs(tmp):
    """name -> (oracle cascade, [oracle result per frame]): computed once per cascade and shared, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            o = ce.oracle_cascade(tmp, name)
            res = []
            for img, sf in ce.frames(name):
                ref = orc.detect_raw(o, img, sf, nthreads=8, full=True)
                res.append((ref, orc.group_rectangles(ref.candidates[:, 3:7], 2, 0.2)))
            cache[name] = (o, res)
        return cache[name]
    return get


def _classifier(name, **kw):
    p = cc.CascadeClassifier(**kw)
    assert p.load_from_string(ce.built(name).xml), getattr(p, "load_error", "")
    return p


def _same_as_oracle(p, name, refs, frames=(0, 1)):
    o, res = refs(name)
    n = 0
    for i in frames:
        img, sf = ce.frames(name)[i]
        ref, grouped = res[i]
        codes, sums, vis = p.debug_windows(img, sf)
        assert len(codes) == ref.n_grid_windows
        bad = np.nonzero(codes != ref.codes)[0]
        assert len(bad) == 0, f"{name}: {len(bad)} of {len(codes)} window results differ, first at {bad[:5].tolist()}: {codes[bad[:5]].tolist()} for {ref.codes[bad[:5]].tolist()}"
        bad = np.nonzero(sums != ref.sums)[0]
        assert len(bad) == 0, f"{name}: {len(bad)} stage sums differ, first {sums[bad[:3]].tolist()} for {ref.sums[bad[:3]].tolist()} (codes {codes[bad[:3]].tolist()})"
        assert (vis == ref.visited).all()
        raw = p.detect_raw(img, sf)
        assert raw.shape == ref.candidates.shape and (raw == ref.candidates).all()
        got = p.detectMultiScale(img, sf, 2)
        assert got.shape == grouped.shape and (got == grouped).all()
        n += len(raw)
    assert n > 0
    return n


def _coverable(o, k):
    """Stages that specialize(k) compiles: whole stages within the stump budget."""
    n, stumps = 0, 0
    while n < o.nstages and n < k and (n == 0 or stumps + int(o.stage_ntrees[n]) <= SPEC_BUDGET):
        stumps += int(o.stage_ntrees[n])
        n += 1
    return n


# ------------------------------------------------------------------ table-driven detector
@pytest.mark.parametrize("name", ce.NAMES)
def test_table_driven_detector(refs, name):
    _same_as_oracle(_classifier(name), name, refs)


@pytest.mark.parametrize("name", ce.G_NAMES)
def test_single_stage_cascades(refs, name):
    """One stage: the dense phase emits the candidates itself. Table-driven kernel, and for the stump cascades the
    specialised one (LBP: the rolled dense loop of the module with 20-row tiles)."""
    p = _classifier(name)
    _same_as_oracle(p, name, refs, frames=(0,))
    if ce.ONE_STAGE[name][1]:
        assert p.specialize(1) == 1 and p.specialized_stages() == 1
        _same_as_oracle(p, name, refs, frames=(0,))


SWITCHED = ["a_below_quarter", "a_between", "a_at_bound", "e_sizes_small", "e_sizes_large"]


@pytest.mark.parametrize("wave_below,split", [(0, 1), (64, 1), (0, 0), (64, 0)])
@pytest.mark.parametrize("name", SWITCHED)
def test_wave_phase_and_stump_split_switches(refs, name, wave_below, split, monkeypatch):
    """The wavefront-per-window phase off and at its widest, the stump split on and off: late stages of 1 to 129 stumps and
    the critical stages of the order-independence cascades. (a_at_bound is not order-independent: the switches must be
    ignored for it, the sums stay sequential.)"""
    monkeypatch.setenv("CCAMD_WAVE_BELOW", str(wave_below))
    monkeypatch.setenv("CCAMD_SPLIT_STUMPS", str(split))
    _same_as_oracle(_classifier(name), name, refs, frames=(0,))


# ------------------------------------------------------------------ specialised detector
def _specialised(name, k, refs, monkeypatch, env=(), batch=True):
    for kk, v in env:
        monkeypatch.setenv(kk, v)
    o, _ = refs(name)
    p = _classifier(name)
    want = _coverable(o, k)
    assert p.specialize(k) == want and p.specialized_stages() == want
    _same_as_oracle(p, name, refs)
    if batch:  # the batch path against the table-driven kernel
        frames = np.stack([ce.frames(name)[0][0][:200, :304], ce.frames(name)[0][0][100:300, 96:400], ce.frames(name)[0][0][50:250, 40:344]])
        spec = p.detect_batch(frames, 1.2, 2)
        assert p.specialize(0) == 0
        plain = p.detect_batch(frames, 1.2, 2)
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(spec, plain)) and sum(len(a) for a in plain) > 0
    return want


SPEC_NAMES = [n for n in ce.NAMES if n not in ce.D_NAMES]


@pytest.mark.parametrize("name", SPEC_NAMES)
def test_specialised_through_the_critical_stage(refs, name, monkeypatch):
    """specialize(k) with k past the critical stage: every stage the stump budget allows is generated code."""
    b = ce.built(name)
    got = _specialised(name, b.nstages, refs, monkeypatch)
    assert got > b.critical, "the critical stage is generated code"


@pytest.mark.parametrize("name", SPEC_NAMES)
def test_specialised_up_to_the_critical_stage(refs, name, monkeypatch):
    """specialize(k) stopping one stage before the critical one: it runs from the tables, behind generated stages."""
    b = ce.built(name)
    assert _specialised(name, b.critical, refs, monkeypatch, batch=False) == b.critical


@pytest.mark.parametrize("name", ["a_below_quarter", "b_below", "c_128x40"])
def test_specialised_without_corner_sharing(refs, name, monkeypatch):
    """CCAMD_SPEC_NO_SHARE=1: the generated stages in file order, every corner read."""
    _specialised(name, ce.built(name).nstages, refs, monkeypatch, env=(("CCAMD_SPEC_NO_SHARE", "1"),), batch=False)


@pytest.mark.parametrize("name", ce.D_NAMES)
@pytest.mark.parametrize("k", [3, 2])
def test_specialised_16_bit_tiles(refs, name, k, monkeypatch):
    """CCAMD_SPEC_TILE16=1: value ranges of 32640 (the sign-extended 16-bit form) and 32895 (strips), rectangles of 256 and
    258 to 264 pixels on either side of the strip cutter's limit, one-pixel rows and columns across the window; generated
    stages and, behind them, table-driven stages that read the 32-bit integral from global memory."""
    _specialised(name, k, refs, monkeypatch, env=(("CCAMD_SPEC_TILE16", "1"),), batch=(k == 3))


# ------------------------------------------------------------------ training side
MINED = ce.A_NAMES + ce.B_NAMES + ce.C_NAMES + ce.E_HAAR_NAMES + [ce.REFUSED] + ce.E_LBP_NAMES + ce.F_NAMES


@pytest.mark.parametrize("name", MINED)
def test_negative_miner(tmp, name):
    """NegativeMiner.run on the cascade's first frame at two offsets: the flags of orc.negmine_image. The miner has no stage
    limit: the cascade of 64 stages is served too."""
    b = ce.built(name)
    path = ce.hw.write_xml(tmp, b.xml, name + "_mine.xml")
    o = orc.load_cascade_xml(path)
    c = cc.CascadeClassifier(path)
    assert not c.empty(), getattr(c, "load_error", "")
    m = cc.NegativeMiner(c)
    img = ce.frames(name)[0][0]
    total = 0
    for ox, oy in ((0, 0), (5, 3)):
        want_f, want_p, want_i = orc.negmine_image(o, img, ox, oy, max_keep=40)
        got_f, got_p, got_i = m.run(img, ox, oy, max_keep=40)
        assert got_f.shape == want_f.shape and (got_f == want_f).all(), f"{(got_f != want_f).sum()} of {len(want_f)} windows differ"
        assert (got_i == want_i).all() and (got_p == want_p).all()
        total += int(want_f.sum())
        assert want_f.sum() < len(want_f)
    # (the trainer goes left on v <= thr: on the node-tie cascade, whose thresholds were set for v < thr, no window passes)
    assert total > 0 or name.startswith("f_node_ties")


@pytest.mark.parametrize("name", MINED)
def test_training_side_predict(tmp, name):
    """predict_cascade on about 500 windows cut from the cascade's first frame against orc.train_predict."""
    b = ce.built(name)
    path = ce.hw.write_xml(tmp, b.xml, name + "_predict.xml")
    o = orc.load_cascade_xml(path)
    c = cc.CascadeClassifier(path)
    imgs = ce.sample_windows(name)
    haar = b.kind == "haar"
    tilted = haar and bool(o.haar["tilted"].any())
    e = cc.CvFeatureEvaluator.create(ev.HAAR if haar else ev.LBP)
    e.init(cc.CvFeatureParams(ev.HAAR if haar else ev.LBP, ev.ALL if tilted else ev.BASIC), len(imgs), (b.W, b.H))
    e.setImages(imgs)
    got = e.predict_cascade(c)
    s, t, nf = orc.set_images(imgs, want_tilted=tilted, want_norm=haar)
    want = np.array([orc.train_predict(o, s, t, nf, i, b.W, b.H) for i in range(len(imgs))], np.uint8)
    assert (got == want).all(), f"{(got != want).sum()} of {len(want)} samples differ"
    # (v <= thr on the trainer's side: of the Haar tie cascades, whose thresholds were set for v < thr, no sample passes)
    assert want.sum() < len(imgs) and (want.sum() > 0 or name in ("f_node_ties", "f_node_ties_plain", "f_stage_ties"))


# ------------------------------------------------------------------ the stage limit
def test_64_stages_are_refused_and_63_served(refs):
    p = _classifier(ce.REFUSED)
    img, sf = ce.frames(ce.REFUSED)[0]
    for call in (lambda: p.detectMultiScale(img, sf, 2), lambda: p.detect_raw(img, sf), lambda: p.specialize(2)):
        with pytest.raises(cc.CascadeError, match=r"cascades with 64 stages are not supported \(limit 63\)") as e:
            call()
        assert e.value.status == L.CC_ERR_UNSUPPORTED
    # a detector created afterwards works, up to the last of 63 stages
    _same_as_oracle(_classifier("e_63_stages"), "e_63_stages", refs, frames=(1,))
    o, res = refs("e_63_stages")
    assert (res[1][0].codes == -62).any() and (res[1][0].codes == -56).any()
