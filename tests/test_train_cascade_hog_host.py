"""The inputs of the HOG train_cascade tests (tests/hog_train_cases.py), run through the witness driver on the CPU with libm's
exp: the recipe of the positives must leave the witness at least two stages to train, windows to reject, stages that span
images and a stage that resumes in the middle of one. A change of the recipe is caught here, without a GPU. Also the XML
parser and the witness's model against each other: the cascade written from the witness's stages walks as the witness does."""
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import evaluator as ev
from cascadeclassifier_amd import trainer
from tests import boost_witness as bw
from tests import hog_cascade_factory as hf
from tests import hog_restatement as hog
from tests import hog_train_cases as tc


@pytest.fixture(scope="module", params=tc.CASES, ids=tc.case_id)
def run(request):
    win, depth, amplitude = request.param
    pos = tc.positives(win, amplitude)
    return (win, depth, pos) + tc.witness_train(pos, tc.backgrounds(), win, depth, bw.libm_exp)


def test_inputs_are_worth_training_on(run):
    win, depth, pos, stages, records, end, notes = run
    print(end, [(r["neg_count"], r["neg_consumed"], r["acceptance_ratio"]) for r in records], notes)
    tc.assert_worth_training(records, notes)
    assert end == trainer.END_NUM_STAGES and len(stages) == tc.NUM_STAGES
    assert all(len(r["weak"]) <= tc.PARAMS["max_weak_count"] for r in records)
    if depth > 1:
        assert any(len(w["nodes"]) > 1 for _, weak in stages for w in weak), "no tree deeper than a stump"


def test_stump_case_at_24x24_consumes_what_the_recipe_was_chosen_for():
    """24x24 stumps at amplitude 30: three stages that consume 60, 120 and 368 windows over 1, 3 and 5 images."""
    win, depth, amplitude = tc.CASES[0]
    assert (win, depth, amplitude) == ((24, 24), 1, 30)
    _, records, _, notes = tc.witness_train(tc.positives(win, amplitude), tc.backgrounds(), win, depth, bw.libm_exp)
    assert [r["neg_consumed"] for r in records] == [60, 120, 368] and [n["images"] for n in notes] == [1, 3, 5]


def test_written_cascade_names_the_witness_s_variables(run):
    """from_stumps / from_trees of the witness's stages (host only), read back by the tests' own parser: every <rect> is the
    catalog block and component of the variable the witness chose, and the file's stages walk the positives as the
    witness's model does."""
    win, depth, pos, stages, records, end, notes = run
    build = cc.CascadeClassifier.from_trees if depth > 1 else cc.CascadeClassifier.from_stumps
    text = tc.saved_text(build(ev.HOG, win, stages))
    tc.assert_xml_is_the_witness(text, win, stages)
    W, H, feats, parsed = hf.parse_hog_xml(text)
    hist, norm = hog.set_images(pos)
    by_file = hf.stage_walk(hf.parsed_model(parsed), hf.feature_values(feats, hist, norm))
    by_witness = hf.stage_walk(tc.model_of(stages), tc.all_values(pos, hog.catalog(*win)))
    assert (by_file == by_witness).all() and by_witness.sum() >= tc.NUM_POS
