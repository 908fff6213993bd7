"""cc_cascade_from_trees under AddressSanitizer + UBSan: tests/cpp/trees_host.cpp, a stand-alone program compiled with g++
against the product's host sources (CPU build only), builds cascades of trees from random and from hostile arguments."""
import subprocess

from tests.host_build import build_program


def test_from_trees_never_trips_a_sanitizer(tmp_path):
    out = build_program("trees_host", tmp_path)
    r = subprocess.run([out, "600", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "built" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
