"""The numpy witness of the sample synthesis against the reference's recorded output (tests/golden/barcode.vec is the
expected_barcode.vec of the reference's createsamples README), and its two forms against each other."""
import numpy as np
import pytest

from tests import sample_witness as W
from tests.sample_cases import BARCODE, CASES, barcode_image, barcode_vec_samples, obj_image


def test_sparse_witness_reproduces_the_recorded_vec():
    got = W.generate(barcode_image(), 100, 75, 32, W.Params(**BARCODE), W.RNG(12345))
    want = barcode_vec_samples()
    assert got.shape == want.shape and (got == want).all(), f"{(got != want).sum()} of {want.size} bytes differ"


def test_dense_witness_reproduces_the_first_samples():
    got = W.generate(barcode_image(), 3, 75, 32, W.Params(**BARCODE), W.RNG(12345), dense=True)
    assert (got == barcode_vec_samples()[:3]).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_and_sparse_agree(name):
    sw, sh, ow, oh, kw = CASES[name]
    img = obj_image(sw, sh, 5, kw.get("bgcolor", 0))
    bg = np.random.RandomState(3).randint(0, 256, (6, oh, ow)).astype(np.uint8)
    a = W.generate(img, 6, ow, oh, W.Params(**kw), W.RNG(12345), backgrounds=bg, dense=True)
    b = W.generate(img, 6, ow, oh, W.Params(**kw), W.RNG(12345), backgrounds=bg)
    assert (a == b).all()
    assert len(np.unique(a)) > 8  # not a flat picture
