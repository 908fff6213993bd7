"""cc_cascade_from_trees under AddressSanitizer + UBSan: tests/cpp/trees_host.cpp, a stand-alone program compiled with g++
against the product's host sources (CPU build only), builds cascades of trees from random and from hostile arguments."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cascadeclassifier_amd", "csrc")


def test_from_trees_never_trips_a_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path / "trees_host")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "trees_host.cpp")] + [os.path.join(CSRC, f) for f in ("cc_xml.cpp", "cc_cascade.cpp", "cc_host.cpp")] + \
          ["-o", out, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([out, "600", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "built" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
