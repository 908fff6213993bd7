"""The readers and writers of the trainer's files (params.xml, stage<i>.xml; section 6d of the C ABI) under
AddressSanitizer + UBSan, as tests/test_host_sanitizers.py holds the cascade reader: tests/cpp/fuzz_trainfiles.cpp is a
stand-alone program compiled with g++ against the product's host sources and run on the CPU."""
import subprocess

import pytest

from tests.host_build import build_program


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    return build_program("fuzz_trainfiles", tmp_path_factory.mktemp("fuzz"))


def test_mutated_training_files_never_trip_a_sanitizer(fuzz_bin, tmp_path):
    r = subprocess.run([fuzz_bin, "3000", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    read, refused = (int(v) for v in r.stdout.split("stages: ")[1].split(";")[0].replace(" read, ", " ").replace(" refused", "").split())
    assert read > 100 and refused > 100, r.stdout  # the mutants reached both ends of the reader
