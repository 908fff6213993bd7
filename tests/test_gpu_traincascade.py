"""The traincascade driver and tool (cascadeclassifier_amd/traincascade.py) on the smallest case of
tests/test_gpu_train_cascade.py: a run that was interrupted after any stage and called again leaves the files, and returns
the records, of the run that was not; what the directory holds decides where a run starts; the tool prints the transcript
and writes the driver's files."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from cascadeclassifier_amd import samples as sm
from cascadeclassifier_amd import traincascade as tc
from cascadeclassifier_amd import trainer
from cascadeclassifier_amd.detector import vec_write
from oracle import oracle as orc
from tests.test_gpu_train_cascade import NUM_NEG, NUM_POS, NUM_STAGES, PARAMS, WIN, _backgrounds, _positives
from tests.util import frame_natural

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"lbp": dict(feature_type=ev.LBP), "haar_basic": dict(feature_type=ev.HAAR, haar_mode=ev.BASIC), "lbp_depth2": dict(feature_type=ev.LBP, max_depth=2)}


class Stop(Exception):
    pass


def _inputs():
    return _positives(80, 17), _backgrounds()


def _run(data_dir, config, num_stages=NUM_STAGES, stop_after=None, **over):
    """train_cascade_dir on the shared inputs; stop_after = i: on_stage raises Stop behind stage i. Returns its result and stdout's lines."""
    lines = []

    def on_stage(i, record, cascade):
        if i == stop_after:
            raise Stop()
    positives, backgrounds = _inputs()
    kw = dict(PARAMS, win=WIN, on_stage=on_stage, log=lines.append, **CONFIGS[config])
    kw.update(over)
    return tc.train_cascade_dir(str(data_dir), positives, backgrounds, NUM_POS, NUM_NEG, num_stages, **kw), lines


_A = {}


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """config -> (directory, (cascade, loaded, records, end), lines) of the uninterrupted run, made once per config and left unchanged."""
    def get(config):
        if config not in _A:
            d = tmp_path_factory.mktemp("a_" + config)
            result, lines = _run(d, config)
            assert result[1] == 0 and result[3] == trainer.END_NUM_STAGES and len(result[2]) == NUM_STAGES
            assert sorted(os.listdir(d)) == ["cascade.xml", "params.xml", "resume.json"] + ["stage%d.xml" % i for i in range(NUM_STAGES)]
            _A[config] = (str(d), result, lines)
        return _A[config]
    return get


def _same(a, b, where=()):
    """equality of records, field by field, tolerance 0"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), where
        for k in a:
            _same(a[k], b[k], where + (k,))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, where + (k,))
    elif a is None or b is None:
        assert a is None and b is None, where
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype and (x == y).all(), (where, a, b)


def _files_equal(a, b, names=None):
    names = names or ["cascade.xml", "params.xml"] + ["stage%d.xml" % i for i in range(NUM_STAGES)]
    for n in names:
        assert open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read(), n


def _copy(src, dst, names):
    os.makedirs(dst, exist_ok=True)
    for n in names:
        shutil.copy(os.path.join(src, n), os.path.join(dst, n))


@pytest.mark.parametrize("config,k", [("lbp", 1), ("lbp", 2), ("haar_basic", 1), ("haar_basic", 2), ("lbp_depth2", 1)])
def test_an_interrupted_run_equals_the_uninterrupted_one(config, k, run_a, tmp_path):
    a, (_, _, a_records, _), _ = run_a(config)
    b = str(tmp_path / "b")
    with pytest.raises(Stop):
        _run(b, config, stop_after=k - 1)
    assert sorted(os.listdir(b)) == ["params.xml", "resume.json"] + ["stage%d.xml" % i for i in range(k)]  # no cascade.xml, no temporary file
    (cascade, loaded, records, end), lines = _run(b, config)
    assert loaded == k and end == trainer.END_NUM_STAGES
    _files_equal(a, b)
    _same(records, a_records[k:])
    assert lines[:4] == tc.BANNER and ("Stage 0 is loaded" if k == 1 else "Stages 0-%d are loaded" % (k - 1)) in lines
    if config == "lbp_depth2":
        assert cascade.info()["max_nodes_per_tree"] > 1
    if (config, k) == ("lbp", 2):
        # a kill between resume.json and the stage file: resume.json already knows of two stages, one is on disk
        os.remove(os.path.join(b, "stage1.xml"))
        os.remove(os.path.join(b, "cascade.xml"))
        (_, loaded, records, _), _ = _run(b, config)
        assert loaded == 1
        _files_equal(a, b)
        _same(records, a_records[1:])


def test_without_resume_json_the_reader_starts_afresh(run_a, tmp_path, capfd):
    """A directory as the reference's tool leaves it: the loaded stages go on with the reader at its first image."""
    k = 1
    a, (_, _, a_records, _), _ = run_a("lbp")
    b = str(tmp_path / "b")
    _copy(a, b, ["params.xml"] + ["stage%d.xml" % i for i in range(k)])
    capfd.readouterr()
    (cascade, loaded, records, end), _ = _run(b, "lbp")
    assert loaded == k and "resume.json is missing" in capfd.readouterr().err
    positives, backgrounds = _inputs()
    initial = [tc.read_stage(os.path.join(a, "stage%d.xml" % i), ev.LBP) for i in range(k)]
    w_cascade, w_records, w_end = cc.train_cascade(positives, backgrounds, NUM_POS, NUM_NEG, NUM_STAGES, win=WIN, feature_type=ev.LBP,
                                                   initial_stages=initial, **PARAMS)
    assert end == w_end
    _same(records, w_records)
    p = tc.read_params(os.path.join(a, "params.xml"))
    w_cascade.save(str(tmp_path / "w.xml"), params=p)
    assert open(os.path.join(b, "cascade.xml"), "rb").read() == open(tmp_path / "w.xml", "rb").read()
    print("neg_consumed of stage %d: fresh reader %d, continued reader %d" % (k, records[0]["neg_consumed"], a_records[k]["neg_consumed"]))
    assert records[0]["neg_consumed"] != a_records[k]["neg_consumed"]  # or the two readers could not be told apart
    # a resume.json of another background list or window, or without the entry, is not used either
    for broken in ('{"backgrounds": 5, "window": [24, 24], "1": {}}', '{"backgrounds": 4, "window": [24, 24]}', "not json",
                   '{"backgrounds": 4, "window": [24, 24], "2": {"last": 9,"round": 0, "current": 0, "offset": [0, 0], "position": 0}}'):
        c = str(tmp_path / ("c%d" % len(broken)))
        _copy(a, c, ["params.xml", "stage0.xml", "stage1.xml"])
        open(os.path.join(c, "resume.json"), "w").write(broken)
        result, _ = _run(c, "lbp", num_stages=2)  # nothing to train: the reader is set up and left alone
        assert result[1] == 2 and "the background reader starts at the first image" in capfd.readouterr().err


def test_empty_initial_stages_and_a_fresh_reader_change_nothing(run_a, tmp_path):
    a, (a_cascade, _, a_records, a_end), _ = run_a("lbp")
    positives, backgrounds = _inputs()
    reader = cc.BackgroundReader(backgrounds, WIN)
    states = []
    cascade, records, end = cc.train_cascade(positives, backgrounds, NUM_POS, NUM_NEG, NUM_STAGES, win=WIN, feature_type=ev.LBP, initial_stages=[],
                                             reader=reader, on_stage=lambda i, rec, c: states.append(reader.state()), **PARAMS)
    assert end == a_end
    _same(records, a_records)
    cascade.save(str(tmp_path / "c.xml"))
    a_cascade.save(str(tmp_path / "a.xml"))
    assert open(tmp_path / "c.xml", "rb").read() == open(tmp_path / "a.xml", "rb").read()
    import json
    saved = json.load(open(os.path.join(a, "resume.json")))
    assert [dict(s, offset=list(s["offset"])) for s in states] == [saved[str(i + 1)] for i in range(NUM_STAGES)]
    assert (saved["backgrounds"], saved["window"]) == (len(backgrounds), list(WIN))


def test_fewer_stages_than_files_trains_nothing(run_a, tmp_path):
    a, _, _ = run_a("lbp")
    b = str(tmp_path / "b")
    _copy(a, b, ["params.xml", "resume.json"] + ["stage%d.xml" % i for i in range(NUM_STAGES)])
    (cascade, loaded, records, end), lines = _run(b, "lbp", num_stages=2)
    assert (loaded, records, end) == (2, [], trainer.END_NUM_STAGES) and cascade.info()["n_stages"] == 2
    assert "Stages 0-1 are loaded" in lines and not any("TRAINING" in l for l in lines)
    two = [tc.read_stage(os.path.join(a, "stage%d.xml" % i), ev.LBP) for i in range(2)]
    cc.CascadeClassifier.from_stumps(ev.LBP, WIN, two).save(str(tmp_path / "two.xml"), params=tc.read_params(os.path.join(a, "params.xml")))
    assert open(os.path.join(b, "cascade.xml"), "rb").read() == open(tmp_path / "two.xml", "rb").read()
    _files_equal(a, b, ["params.xml"] + ["stage%d.xml" % i for i in range(NUM_STAGES)])  # nothing else was touched


def test_preloaded_parameters_win(run_a, tmp_path):
    a, (_, _, a_records, _), _ = run_a("lbp")
    b = str(tmp_path / "b")
    _copy(a, b, ["params.xml", "resume.json", "stage0.xml", "stage1.xml"])
    (cascade, loaded, records, end), lines = _run(b, "lbp", max_weak_count=5, boost_type=ev.BOOST_REAL)
    assert loaded == 2 and lines[:4] == tc.BANNER and "boostType: GAB" in lines and "maxWeakCount: %d" % PARAMS["max_weak_count"] in lines
    _files_equal(a, b)
    _same(records, a_records[2:])
    # a stage file that does not parse is an error that names it; the reference would train the stage again
    open(os.path.join(b, "stage2.xml"), "w").write("<opencv_storage><stage2>")
    with pytest.raises(cc.CascadeError, match="stage2.xml"):
        _run(b, "lbp")
    # stage files without params.xml are ignored
    os.remove(os.path.join(b, "params.xml"))
    (_, loaded, _, _), _ = _run(b, "lbp", num_stages=1)
    assert loaded == 0


def test_base_format_save(run_a, tmp_path):
    a, _, _ = run_a("haar_basic")
    b = str(tmp_path / "b")
    _copy(a, b, ["params.xml", "resume.json"] + ["stage%d.xml" % i for i in range(NUM_STAGES)])
    (cascade, loaded, records, _), _ = _run(b, "haar_basic", base_format_save=True)
    assert loaded == NUM_STAGES and records == []
    stages = [tc.read_stage(os.path.join(a, "stage%d.xml" % i), ev.HAAR) for i in range(NUM_STAGES)]
    cc.CascadeClassifier.from_stumps(ev.HAAR, WIN, stages, haar_mode=ev.BASIC).save(str(tmp_path / "legacy.xml"), baseFormat=True)
    text = open(os.path.join(b, "cascade.xml"), "rb").read()
    assert text == open(tmp_path / "legacy.xml", "rb").read() and b"opencv-haar-classifier" in text
    c = str(tmp_path / "c")
    with pytest.raises(cc.CascadeError, match="old file format is used for Haar-like features only"):
        _run(c, "lbp", base_format_save=True)
    assert not os.path.exists(c) or os.listdir(c) == []
    with pytest.raises(cc.CascadeError, match="LOGIT"):
        _run(c, "lbp", boost_type=ev.BOOST_LOGIT)
    assert not os.path.exists(c) or os.listdir(c) == []


def _tool(args, timeout=300):
    return subprocess.run([sys.executable, "-m", "cascadeclassifier_amd.traincascade"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def _mask(lines):
    return [re.sub(r"^(Precalculation time: |Training until now has taken ).*$", r"\1*", l) for l in lines]


def test_the_tool_end_to_end(run_a, tmp_path):
    a, (_, _, a_records, a_end), _ = run_a("lbp")
    positives, backgrounds = _inputs()
    vec, bg = str(tmp_path / "pos.vec"), str(tmp_path / "bg.txt")
    vec_write(vec, positives, WIN[0], WIN[1])
    for k, im in enumerate(backgrounds):
        sm.write_gray(str(tmp_path / ("bg%d.pgm" % k)), im)
    open(bg, "w").write("".join("bg%d.pgm\n" % k for k in range(len(backgrounds))))
    d = str(tmp_path / "data")
    common = ["-vec", vec, "-bg", bg, "-numPos", str(NUM_POS), "-numNeg", str(NUM_NEG), "-numStages", str(NUM_STAGES), "-featureType", "LBP",
              "-w", str(WIN[0]), "-h", str(WIN[1]), "-maxWeakCount", str(PARAMS["max_weak_count"]), "-numThreads", "3"]
    r = _tool(["-data", d] + common)
    assert r.returncode == 0, r.stderr
    _files_equal(a, d)
    e = cc.CvFeatureEvaluator.create(ev.LBP)
    e.init(cc.CvFeatureParams(ev.LBP, ev.BASIC), 1, WIN)
    want = tc.transcript(data_dir=d, vec_name=vec, bg_name=bg, num_pos=NUM_POS, num_neg=NUM_NEG, num_stages=NUM_STAGES,
                         params=tc.read_params(os.path.join(a, "params.xml")), n_features=e.getNumFeatures(), records=a_records, end=a_end)
    assert _mask(r.stdout.splitlines()) == _mask(want)
    # LOGIT boost: the library's message, and the directory is not made
    d2 = str(tmp_path / "data_lb")
    r = _tool(["-data", d2, "-bt", "LB"] + common)
    assert r.returncode != 0 and "LOGIT" in r.stderr and not os.path.exists(d2)
    # the positives run out
    short = str(tmp_path / "short.vec")
    vec_write(short, positives[:NUM_POS - 1], WIN[0], WIN[1])
    r = _tool(["-data", str(tmp_path / "data_short")] + common[:1] + [short] + common[2:])
    assert r.returncode == 1 and "Can not get new positive sample. vec-file is over." in r.stderr
    # a .vec of another sample size
    r = _tool(["-data", str(tmp_path / "data_size")] + common + ["-w", "20"])
    assert r.returncode == 1 and "needs 480" in r.stderr


def test_the_resumed_cascade_against_the_oracle(run_a, tmp_path):
    """The cascade assembled from stage files: the detector and the trainer's predict against the oracle on its cascade.xml."""
    a, _, _ = run_a("lbp_depth2")
    b = str(tmp_path / "b")
    _copy(a, b, ["params.xml", "resume.json", "stage0.xml", "stage1.xml"])
    (cascade, loaded, _, _), _ = _run(b, "lbp_depth2")
    assert loaded == 2
    path = os.path.join(b, "cascade.xml")
    back, o = cc.CascadeClassifier(path), orc.load_cascade_xml(path)
    assert back.info() == cascade.info() and back.train_params() == tc.read_params(os.path.join(b, "params.xml")).as_dict()
    positives, backgrounds = _inputs()
    rng = np.random.default_rng(5)
    crops = [backgrounds[0][y:y + WIN[1], x:x + WIN[0]] for x, y in zip(rng.integers(0, 150, 60), rng.integers(0, 100, 60))]
    samples = np.concatenate([positives[:40], np.stack(crops)])
    e = cc.CvFeatureEvaluator.create(ev.LBP)
    e.init(cc.CvFeatureParams(ev.LBP, ev.BASIC), len(samples), WIN)
    e.setImages(samples)
    s, t, nf = orc.set_images(samples, want_tilted=False, want_norm=False)
    want = np.array([orc.train_predict(o, s, t, nf, k, WIN[0], WIN[1]) for k in range(len(samples))], np.uint8)
    assert (e.predict_cascade(cascade) == want).all() and (e.predict_cascade(back) == want).all() and 0 < want.sum() < len(samples)
    frame = frame_natural(96, 96, 77)
    frame[30:30 + WIN[1], 40:40 + WIN[0]] = positives[0]
    got_rects = back.detectMultiScale(frame, 1.1, 1)
    want_rects = orc.detect_multiscale(o, frame, 1.1, 1)
    assert got_rects.shape == want_rects.shape and (got_rects == want_rects).all()
