"""Runs the C++ test of the HOG host adaptor (tests/cpp/test_hog_adaptor.cpp): the reference's HOG cases through
CvHOGEvaluator and the writeFeatures format, on the HIP path."""
import os
import subprocess

import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cascadeclassifier_amd", "lib")


def test_hog_adaptor_test_is_built():
    assert os.path.exists(os.path.join(LIB, "test_hog_adaptor")), "run __graft_entry__.build()"


@pytest.mark.gpu
def test_hog_adaptor_cases_pass_on_the_device(tmp_path):
    r = subprocess.run([os.path.join(LIB, "test_hog_adaptor"), os.path.join(str(tmp_path), "hog_features.xml")],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert " 0 failed" in r.stdout
