"""train_cascade (cascadeclassifier_amd/trainer.py) against a driver written here from the reference's text
(cascadeclassifier.cpp:203-284, :308-357) over parts that have tests of their own: NegReader window by window
(tests/fill_witness.py), the oracle's reader loop for the flags and pixels of an image's windows, setImages, CascadeBoost and
from_stumps. Counts, acceptance ratios, weak records, the saved XML and the reason training ended must be equal, for any
batch size of the driver."""
import math
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import evaluator as ev
from cascadeclassifier_amd import trainer
from oracle import oracle as orc
from tests import cascade_factory as cf
from tests import fill_witness as fw
from tests.util import frame_natural

pytestmark = pytest.mark.gpu

WIN = (24, 24)
NUM_POS = NUM_NEG = 60
NUM_STAGES = 3
PARAMS = dict(boost_type=ev.BOOST_GENTLE, min_hit_rate=0.995, max_false_alarm=0.5, weight_trim_rate=0.95, max_weak_count=3)


def _positives(n, seed):
    """Windows of natural frames with a faint pattern on top: no single stump separates them from the backgrounds, so a
    stage of three stumps lets a good share of the background windows through and the next stage has work to do."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:WIN[1], 0:WIN[0]]
    pattern = 40 * np.sin(xx / WIN[0] * 3.1) * np.cos(yy / WIN[1] * 2.3)
    frame = frame_natural(400, 300, seed).astype(np.float64)
    out = []
    for _ in range(n):
        x, y = int(rng.integers(0, 400 - WIN[0])), int(rng.integers(0, 300 - WIN[1]))
        out.append(np.clip(frame[y:y + WIN[1], x:x + WIN[0]] + pattern + rng.normal(0, 6, (WIN[1], WIN[0])), 0, 255))
    return np.stack(out).astype(np.uint8)


def _backgrounds():
    return [frame_natural(176, 132, 31), frame_natural(120, 100, 32), frame_natural(176, 132, 33), frame_natural(120, 100, 34)]


def _accept_all(tmp):
    feat = orc.make_haar_feature(False, [(0, 0, 4, 4, -1.0), (0, 0, 2, 2, 4.0)])
    path = os.path.join(tmp, "accept_all.xml")
    open(path, "w").write(cf.haar_xml(np.array([feat]).reshape(1), [(-1e30, [([(0, -1, 0, 0.0)], [1.0, 1.0])])], mode="BASIC", W=WIN[0], H=WIN[1]))
    return orc.load_cascade_xml(path)


def _witness_train(positives, backgrounds, ftype, tmp, acceptance_ratio_break_value=-1.0):
    reader = fw.NegReaderWitness(backgrounds, WIN)
    required = math.pow(float(np.float32(PARAMS["max_false_alarm"])), float(NUM_STAGES))
    e_pos = cc.CvFeatureEvaluator.create(ftype)
    e_pos.init(cc.CvFeatureParams(ftype, ev.BASIC), len(positives), WIN)
    e_pos.setImages(positives)
    stages, records, notes = [], [], []
    cascade, oracle = None, _accept_all(tmp)
    cache = {}

    def windows_of(idx, off):  # flags of the image's stream and the pixels of the windows that pass, by stream position
        key = (len(stages), idx, off)
        if key not in cache:
            f, kept, pos = orc.negmine_image(oracle, backgrounds[idx], off[0], off[1], max_keep=1 << 16)
            cache[key] = (f, {int(p): kept[r] for r, p in enumerate(pos)})
        return cache[key]

    end = trainer.END_NUM_STAGES
    for i in range(NUM_STAGES):
        flags = np.ones(len(positives), np.uint8) if cascade is None else e_pos.predict_cascade(cascade)
        pos_count, pos_consumed, _, keep = fw.fill_select(flags, 0, NUM_POS)
        if pos_count < NUM_POS:
            raise ValueError("Can not get new positive sample. vec-file is over.")
        pro_num_neg = int(round((float(NUM_NEG) * float(pos_count)) / NUM_POS))
        note = {"resumed_mid_image": reader.img is not None and reader.i != 0, "images": 0}
        got, consumed, neg, last_image = 0, 0, [], None
        for _ in range(pro_num_neg):  # fillPassedSamples, :329-357
            by_ratio = False
            while True:
                if consumed != 0 and float(got + 1) / float(consumed) <= required:
                    by_ratio = True
                    break
                idx, off, wi, _, _ = reader.get()
                consumed += 1
                if (idx, off) != last_image or wi == 0:
                    note["images"] += 1
                    last_image = (idx, off)
                f, pix = windows_of(idx, off)
                if f[wi]:
                    neg.append(pix[wi])
                    got += 1
                    break
            if by_ratio:
                break
        notes.append(note)
        record = {"pos_count": pos_count, "pos_consumed": pos_consumed, "neg_count": got, "neg_consumed": consumed, "acceptance_ratio": None,
                  "weak": None}
        records.append(record)
        if got == 0 and not (consumed > 0 and (float(got) + 1) / float(consumed) <= required):
            end = trainer.END_CANNOT_FILL
            break
        acceptance = 0.0 if consumed == 0 else float(got) / float(consumed)
        record["acceptance_ratio"] = acceptance
        if acceptance <= required:
            end = trainer.END_LEAF_FA_RATE
            break
        if acceptance <= acceptance_ratio_break_value and acceptance_ratio_break_value >= 0:
            end = trainer.END_ACCEPTANCE_BREAK
            break
        samples = np.concatenate([positives[keep], np.stack(neg)])
        labels = np.array([1] * pos_count + [0] * got, np.uint8)
        e = cc.CvFeatureEvaluator.create(ftype)
        e.init(cc.CvFeatureParams(ftype, ev.BASIC), len(samples), WIN)
        e.setImages(samples, labels)
        e.presort()
        weak = cc.CascadeBoost(e, len(samples), **PARAMS).train_stage()
        if not any(w["trained"] for w in weak):
            end = trainer.END_STAGE_NOT_TRAINED
            break
        record["weak"] = weak
        stages.append((weak[-1]["stage_threshold"], weak))
        cascade = cc.CascadeClassifier.from_stumps(ftype, WIN, stages, haar_mode=ev.BASIC)
        path = os.path.join(tmp, "witness_stage%d.xml" % i)
        cascade.save(path)
        oracle = orc.load_cascade_xml(path)
    return cascade, records, end, notes


def _assert_records_equal(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("pos_count", "pos_consumed", "neg_count", "neg_consumed", "acceptance_ratio"):
            assert g[k] == w[k], (i, k, g[k], w[k])
        assert (g["weak"] is None) == (w["weak"] is None), i
        for a, b in zip(g["weak"] or [], w["weak"] or []):
            assert a.keys() == b.keys()
            for k in a:
                same = (np.asarray(a[k]) == np.asarray(b[k])).all()
                assert same, (i, k, a[k], b[k])
        assert len(g["weak"] or []) == len(w["weak"] or [])


@pytest.mark.parametrize("ftype", [ev.HAAR, ev.LBP], ids=["haar_basic", "lbp"])
def test_train_cascade_equals_the_reference_loop(ftype, tmp_path):
    tmp = str(tmp_path)
    positives, backgrounds = _positives(80, 17), _backgrounds()
    w_cascade, w_records, w_end, notes = _witness_train(positives, backgrounds, ftype, tmp)
    summary = [(r["neg_count"], r["neg_consumed"], r["acceptance_ratio"], None if r["weak"] is None else len(r["weak"])) for r in w_records]
    print("witness:", w_end, summary, notes)
    trained = [r for r in w_records if r["weak"] is not None]
    assert len(trained) >= 2, summary
    assert any(n["images"] > 1 for n in notes), notes  # a stage's negatives come from more than one image
    assert any(n["resumed_mid_image"] for n in notes[1:]), notes  # and a stage starts where the one before stopped, mid-image
    w_path = os.path.join(tmp, "witness.xml")
    w_cascade.save(w_path)
    seen = []
    for max_batch in (256, 1):
        cascade, records, end = cc.train_cascade(positives, backgrounds, NUM_POS, NUM_NEG, NUM_STAGES, feature_type=ftype, win=WIN,
                                                 haar_mode=ev.BASIC, max_batch=max_batch, on_stage=lambda i, rec, c: seen.append((max_batch, i)),
                                                 **PARAMS)
        assert end == w_end
        _assert_records_equal(records, w_records)
        path = os.path.join(tmp, "trained_%d.xml" % max_batch)
        cascade.save(path)
        assert open(path, "rb").read() == open(w_path, "rb").read()
    assert seen == [(b, i) for b in (256, 1) for i in range(len(trained))]


def test_positives_running_out_raise(tmp_path):
    positives, backgrounds = _positives(NUM_POS - 1, 17), _backgrounds()
    with pytest.raises(ValueError, match="vec-file is over"):
        cc.train_cascade(positives, backgrounds, NUM_POS, NUM_NEG, 2, feature_type=ev.LBP, win=WIN, **PARAMS)


def test_break_value_ends_training_before_a_stage(tmp_path):
    """acceptanceRatioBreakValue 1.0: stage 0's acceptance ratio is 1 (no stage yet, every window passes), so training ends
    before anything is trained and there is no cascade."""
    positives, backgrounds = _positives(NUM_POS, 17), _backgrounds()
    cascade, records, end = cc.train_cascade(positives, backgrounds, NUM_POS, NUM_NEG, 2, feature_type=ev.LBP, win=WIN,
                                             acceptance_ratio_break_value=1.0, **PARAMS)
    assert cascade is None and end == trainer.END_ACCEPTANCE_BREAK
    assert [(r["neg_count"], r["neg_consumed"], r["acceptance_ratio"], r["weak"]) for r in records] == [(NUM_NEG, NUM_NEG, 1.0, None)]
