"""How the host tests build their stand-alone programs (own main, CPU only): tests/cpp/<name>.cpp against every host source of
the product, with AddressSanitizer + UBSan unless told otherwise."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cascadeclassifier_amd", "csrc")
HOST_SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.cpp")))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_program(name, out_dir, sanitize=True, hip_host_only=False):
    """The path of the program built from tests/cpp/<name>.cpp in out_dir. g++: skips the test when the compiler or the
    sanitizer's runtime is missing. hip_host_only: the host half of a HIP compile (for sources that include device headers)."""
    out = os.path.join(str(out_dir), name)
    if hip_host_only:
        hipcc = HIPCC if os.path.exists(HIPCC) else (shutil.which("hipcc") or HIPCC)
        cmd = [hipcc, "-x", "hip", "--offload-host-only", "-ffp-contract=off"] + [a for f in SANITIZE * sanitize for a in ("-Xarch_host", f)]
    else:
        if shutil.which("g++") is None:
            pytest.skip("g++ not available")
        cmd = ["g++", "-pthread"] + SANITIZE * sanitize
    cmd += ["-std=c++17", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", name + ".cpp")] + HOST_SOURCES + ["-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and not hip_host_only and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out
