"""The readers and writers of the trainer's files (params.xml, stage<i>.xml; section 6d of the C ABI) under
AddressSanitizer + UBSan, as tests/test_host_sanitizers.py holds the cascade reader: tests/cpp/fuzz_trainfiles.cpp is a
stand-alone program compiled with g++ against the product's host sources and run on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cascadeclassifier_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("fuzz") / "fuzz_trainfiles")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "fuzz_trainfiles.cpp")] + [os.path.join(CSRC, f) for f in ("cc_xml.cpp", "cc_cascade.cpp", "cc_host.cpp")] + \
          ["-o", out, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    return out


def test_mutated_training_files_never_trip_a_sanitizer(fuzz_bin, tmp_path):
    r = subprocess.run([fuzz_bin, "3000", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    read, refused = (int(v) for v in r.stdout.split("stages: ")[1].split(";")[0].replace(" read, ", " ").replace(" refused", "").split())
    assert read > 100 and refused > 100, r.stdout  # the mutants reached both ends of the reader
