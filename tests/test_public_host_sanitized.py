"""Host-side memory safety of the public columns' host-only code (the spec
decoder and evaluator of csrc/public_columns.hpp, mlh_system_verify_public in
csrc/verify.cpp), as tests/test_shifted_host_sanitized.py covers the shifted
verifier: a stand-alone program (tests/fuzz/public_verify_asan.cpp) built with
-fsanitize=address,undefined, fed a proof and a spec of the plain-Python model
and run on the CPU over mutants of both.  Nothing is loaded into Python under a
sanitizer."""
import os
import shutil
import struct
import subprocess

import pytest

import public_reference as PUB
from oracle import field as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multilinear_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("public_asan")
    exe = str(d / "public_verify_asan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "fuzz", "public_verify_asan.cpp"),
           os.path.join(CSRC, "verify.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe, d


def dump(name):
    """The model's proof and spec in the driver's input format."""
    mo = PUB.model(name)
    wire, shifts = PUB.program(name)
    b = struct.pack("<6I", mo["log_height"], mo["width"], mo["degree"], mo["pre"], mo["mask"],
                    len(shifts))
    b += struct.pack("<32I", *(shifts + [0] * (32 - len(shifts))))
    b += struct.pack("<2I", len(mo["pcs"]), mo["n_public"])
    b += struct.pack("<I", len(mo["seed"])) + mo["seed"]
    b += struct.pack("<I", len(wire)) + wire
    b += struct.pack("<I", len(mo["wire"])) + mo["wire"]
    b += F.to_bytes(mo["total"]) + F.to_bytes(mo["column_sum"])
    b += mo["coeff_bytes"] + b"".join(F.to_bytes(v) for v in mo["output"])
    b += mo["shift_bytes"] + b"".join(F.to_bytes(v) for v in mo["output2"])
    ncols = [mo["pre"], mo["committed"] - mo["pre"]]
    for group in (mo["pcs"], mo["pcs_shift"]):
        for i, pcs in enumerate(group):
            b += struct.pack("<2I", ncols[i], len(pcs["commitments"]))
            b += pcs["batch_commitment"] + b"".join(pcs["commitments"])
            b += F.to_bytes(pcs["last_elem"]) + pcs["last_random"]
            b += struct.pack("<Q", len(pcs["queries"])) + pcs["queries"]
            b += b"".join(F.to_bytes(a) + F.to_bytes(c) for a, c in pcs["polys"])
    return b + mo["digest"]


@pytest.mark.parametrize("name", ["pfib4", "pmixed5"])
def test_public_verifier_under_asan_ubsan(driver, name):
    exe, d = driver
    seed = d / ("%s.bin" % name)
    seed.write_bytes(dump(name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(seed), "1500"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "public verify ok" in r.stdout
