"""Host-side memory safety of the shifted system proof's host-only code
(mlh_shift_succ_evaluate, mlh_system_verify_shifted in csrc/verify.cpp), as
tests/test_host_sanitized.py covers the other verifiers: a stand-alone program
(tests/fuzz/shifted_verify_asan.cpp) built with -fsanitize=address,undefined,
fed a proof of the plain-Python model and run on the CPU over mutants of it.
Nothing is loaded into Python under a sanitizer."""
import os
import shutil
import struct
import subprocess

import pytest

import shifted_reference as SR
from oracle import field as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multilinear_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("shifted_asan")
    exe = str(d / "shifted_verify_asan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "fuzz", "shifted_verify_asan.cpp"),
           os.path.join(CSRC, "verify.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe, d


def dump(name):
    """The model's proof in the driver's input format."""
    mo = SR.model(name)
    wire, shifts = SR.program(name)
    b = struct.pack("<6I", mo["log_height"], mo["width"], mo["degree"], mo["pre"], mo["mask"],
                    len(shifts))
    b += struct.pack("<32I", *(shifts + [0] * (32 - len(shifts))))
    b += struct.pack("<I", len(mo["pcs"]))
    b += struct.pack("<I", len(mo["seed"])) + mo["seed"]
    b += struct.pack("<I", len(wire)) + wire
    b += F.to_bytes(mo["total"]) + F.to_bytes(mo["column_sum"])
    b += mo["coeff_bytes"] + b"".join(F.to_bytes(v) for v in mo["output"])
    b += mo["shift_bytes"] + b"".join(F.to_bytes(v) for v in mo["output2"])
    ncols = [mo["pre"], mo["width"] - mo["pre"]]
    for group in (mo["pcs"], mo["pcs_shift"]):
        for i, pcs in enumerate(group):
            b += struct.pack("<2I", ncols[i], len(pcs["commitments"]))
            b += pcs["batch_commitment"] + b"".join(pcs["commitments"])
            b += F.to_bytes(pcs["last_elem"]) + pcs["last_random"]
            b += struct.pack("<Q", len(pcs["queries"])) + pcs["queries"]
            b += b"".join(F.to_bytes(a) + F.to_bytes(c) for a, c in pcs["polys"])
    return b + mo["digest"]


@pytest.mark.parametrize("name", ["fib4", "mixed5"])
def test_shifted_verifier_under_asan_ubsan(driver, name):
    exe, d = driver
    seed = d / ("%s.bin" % name)
    seed.write_bytes(dump(name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(seed), "1500"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "shifted verify ok" in r.stdout
