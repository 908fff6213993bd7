"""train_cascade(feature_type=HOG) end to end against the witness driver of tests/hog_train_cases.py, written from the
reference's text (cascadeclassifier.cpp:203-284, :308-357) over yardsticks the library has no part in: the reader witness and
the reader restatement for the window stream, the numpy HOG evaluator for every value, the restated stage walk, BoostWitness /
TreeWitness for the stages. Only the vector exponential is the device's (cc.device_exp), as in the other witness tests.
The end reason, every stage and weak record and the saved XML must be equal, for max_batch 256 and 1; the XML is also read
back by the tests' own parser and held to the witness's variables. The inputs are checked on the CPU in
tests/test_train_cascade_hog_host.py."""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import evaluator as ev
from tests import hog_cascade_factory as hf
from tests import hog_mine_cases as mc
from tests import hog_restatement as hog
from tests import hog_train_cases as tc
from tests import tree_witness as tw

pytestmark = pytest.mark.gpu


def _assert_weak_equal(got, want, where):
    assert len(got) == len(want), where
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), (where, k)
        for name in g:
            if name == "nodes":
                tw.assert_tree_equal(g, w, (where, k))
            else:
                assert (np.asarray(g[name]) == np.asarray(w[name])).all(), (where, k, name, g[name], w[name])


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_hog_train_cascade_equals_the_reference_loop(case):
    win, depth, amplitude = case
    positives, backgrounds = tc.positives(win, amplitude), tc.backgrounds()
    w_stages, w_records, w_end, notes = tc.witness_train(positives, backgrounds, win, depth, cc.device_exp)
    print("witness:", w_end, [(r["neg_count"], r["neg_consumed"], r["acceptance_ratio"]) for r in w_records], notes)
    tc.assert_worth_training(w_records, notes)
    build = cc.CascadeClassifier.from_trees if depth > 1 else cc.CascadeClassifier.from_stumps
    w_text = tc.saved_text(build(ev.HOG, win, w_stages))
    tc.assert_xml_is_the_witness(w_text, win, w_stages)
    for max_batch in (256, 1):
        seen = []
        cascade, records, end = cc.train_cascade(positives, backgrounds, tc.NUM_POS, tc.NUM_NEG, tc.NUM_STAGES, feature_type=ev.HOG, win=win,
                                                 max_depth=depth, max_batch=max_batch, on_stage=lambda i, rec, c: seen.append(i), **tc.PARAMS)
        assert end == w_end and len(records) == len(w_records), (max_batch, end, w_end)
        for i, (g, w) in enumerate(zip(records, w_records)):
            for k in ("pos_count", "pos_consumed", "neg_count", "neg_consumed", "acceptance_ratio"):
                assert g[k] == w[k], (max_batch, i, k, g[k], w[k])
            assert (g["weak"] is None) == (w["weak"] is None), (max_batch, i)
            _assert_weak_equal(g["weak"] or [], w["weak"] or [], (max_batch, i))
        assert seen == list(range(len(w_stages)))
        text = tc.saved_text(cascade)
        assert text.encode() == w_text.encode(), max_batch
        tc.assert_xml_is_the_witness(text, win, w_stages)  # the file itself against the witness, not through from_stumps
        inf = cascade.info()
        assert inf["feature_type"] == ev.HOG and (inf["win_w"], inf["win_h"]) == win and inf["n_stages"] == len(w_stages)
        assert (inf["max_nodes_per_tree"] > 1) == (depth > 1)
    # the trained cascade on the device against the witness's walk: the positives, which mostly pass, and one background's stream
    W, H = win
    cat = hog.catalog(W, H)
    model = tc.model_of(w_stages)
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), len(positives), win)
    e.setImages(positives)
    want = hf.stage_walk(model, tc.all_values(positives, cat))
    assert (e.predict_cascade(cascade) == want).all() and want.sum() >= tc.NUM_POS
    _, wins = mc.reader_stream(backgrounds[0], W, H, 2, 1)
    want = hf.stage_walk(model, tc.all_values(wins, cat))
    got = cc.NegativeMiner(cascade).run(backgrounds[0], 2, 1, max_keep=0)[0]
    assert (got == want).all() and 0 < want.sum() < len(want)
