"""What makes the HOG mining and stage-predict cases (tests/hog_mine_cases.py) worth running on the device, asserted on the
restatement alone: the calibrated cascades let between 10 % and 90 % of the stream through, the long-stage cascade is
order-independent and its long stages both reject and pass windows, the order-dependent cascade is not and its summation order
shows in the flags. The GPU tests (tests/test_gpu_hog_cascade.py) import the same inputs."""
import numpy as np
import pytest

from tests import hog_cascade_factory as hf
from tests import hog_lds_cases as lds
from tests import hog_mine_cases as mc


def _share(flags):
    f = np.concatenate(flags)
    return float(f.sum()) / len(f), len(f)


@pytest.mark.parametrize("depth", [1, 2], ids=["stumps", "trees"])
@pytest.mark.parametrize("win", mc.WINDOWS, ids=lambda w: "%dx%d" % w)
def test_mining_cascades_pass_a_share_of_the_stream(win, depth):
    _, _, stages, flags = mc.mining_case(win, depth)
    share, n = _share(flags)
    print(win, depth, share, n)
    assert 0.10 <= share <= 0.90, (share, n)
    assert n >= 12
    if win in lds.MINER_LARGE:
        assert n <= 60  # one workgroup with 160 KB of LDS and one numpy setImage per window: a few dozen
    if depth == 1:
        assert hf.order_independent(stages)  # the miner's wavefront walk


@pytest.mark.parametrize("depth", [1, 2], ids=["stumps", "trees"])
@pytest.mark.parametrize("win", lds.MINER_WINDOWS, ids=lambda w: "%dx%d" % w)
def test_predict_cascades_pass_a_share_of_the_samples(win, depth):
    samples, _, _, _, flags = mc.predict_case(win, depth)
    assert 0.10 <= float(flags.sum()) / len(samples) <= 0.90


def test_long_stages_reject_and_pass():
    _, _, stages, flags, counts = mc.long_stage_case()
    assert tuple(len(w) for _, w in stages) == mc.LONG_STAGES == (3, 70, 130)
    assert hf.order_independent(stages)
    print(counts.tolist())
    for s in (1, 2):  # the stages whose stumps take a second and a third round of lanes
        entered, passed = counts[s]
        assert passed > 0 and entered - passed > 0, (s, counts.tolist())
    share, _ = _share(flags)
    assert 0.10 <= share <= 0.90


def test_order_dependent_cascade():
    _, _, stages, fwd, rev, wave = mc.order_dependent_case()
    assert not hf.order_independent(stages)
    for _, weaks in stages:  # without the two large votes the stage would be order-independent
        assert hf.order_independent([(0, weaks[1:2] + weaks[3:])]) and not hf.order_independent([(0, weaks[:3])])
        assert len(weaks) < 64  # one stump per lane
    share, n = _share(fwd)
    assert 0.10 <= share <= 0.90, (share, n)
    f, r, w = np.concatenate(fwd), np.concatenate(rev), np.concatenate(wave)
    assert (f != r).sum() > n // 10, "the summation order must be observable on these windows"
    # and the order the device would use if it shared this cascade's stumps among the lanes of a wavefront gives other flags:
    # a miner that took that walk here would fail the GPU test
    print("tree order against wavefront order:", int((f != w).sum()), "of", n, "flags differ")
    assert (f != w).sum() > n // 10


def test_wavefront_order_restated():
    """The restated wavefront sum: equal to the tree-order sum, bit for bit, where the order-independence proof holds (the
    long-stage cascade, whose lanes take up to three stumps each), and the plain total on 64 and 130 distinct integers."""
    _, feats, stages, flags, _ = mc.long_stage_case()
    model = hf.parsed_model(stages)
    for (h, nrm), want in zip(mc.stream_planes((24, 24)), flags):
        vals = hf.feature_values(feats, h, nrm)
        for _, weaks in model["stages"]:
            assert (hf.wave_stage_sums(weaks, vals).view(np.uint64) == hf.stage_sums(weaks, vals).view(np.uint64)).all()
        assert (hf.stage_walk(model, vals, sums=hf.wave_stage_sums) == want).all()
    for k in (1, 5, 64, 130):  # stump t votes 3^(t % 7) * (t + 1): every lane's share matters to the total
        votes = [np.float32(3 ** (t % 7) * (t + 1)) for t in range(k)]
        weaks = [([(0, -1, 0, np.float32(0.5))], [v, v]) for v in votes]
        assert hf.wave_stage_sums(weaks, np.zeros((1, 2), np.float32)).tolist() == [float(sum(float(v) for v in votes))] * 2


def test_predict_case_at_86x85_passes_a_share():
    samples, _, _, stages, flags = mc.predict_case_86x85()
    assert samples.shape == (40, 85, 86) and all(len(nodes) == 1 for _, ws in stages for nodes, _ in ws)
    assert 0.10 <= float(flags.sum()) / len(samples) <= 0.90


def test_order_independence_restated():
    """The bound itself: leaves on a 2^-24 grid with a sum of magnitudes just below and at 2^53 quanta."""
    one = np.float32(1.0)
    assert hf.order_independent([(0, [([(0, -1, 0, 0.5)], [one, -one])] * 100)])
    tiny, big = np.float32(2.0 ** -20), np.float32(2.0 ** 8)  # q = 2^-43: 2^51 quanta per big vote
    below = [([(0, -1, 0, 0.5)], [tiny, tiny])] + [([(0, -1, 0, 0.5)], [big, -big])] * 3
    assert hf.order_independent([(0, below)])
    assert not hf.order_independent([(0, below + [([(0, -1, 0, 0.5)], [big, big])])])
    assert not hf.order_independent([(0, [([(0, -1, 0, 0.5)], [np.float32(np.inf), one])])])
    assert hf.order_independent([(0, [([(0, -1, 0, 0.5)], [np.float32(0), np.float32(0)])])])
