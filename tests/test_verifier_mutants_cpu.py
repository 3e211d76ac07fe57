"""Every check of the host verifiers decides something: csrc/verify.cpp is
built host-only with g++, once as it is and once per mutant (one check taken
out of a copy in the test's temporary directory), and each build is run over
the forged proofs of tests/forge_reference.py.  The unmodified build gives the
oracle's verdict on every member; every mutant accepts at least one member the
oracle rejects.  No sanitizer, nothing preloaded.  CPU only.

The mutant table names exact source text.  When verify.cpp is edited so that
a text no longer occurs the expected number of times, the test fails with
"update the mutant table": that is the price of the guard -- a check that is
rewritten has to be pointed at again, so it cannot silently lose its mutant."""
import concurrent.futures
import ctypes
import os
import shutil
import subprocess

import pytest

import forge_reference as FR
from multilinear_amd import _lib
from test_verifier_forgeries_cpu import VERIFY, c_verdict, phased_status, system_status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multilinear_amd", "csrc")

LAST_RANDOM = "return memcmp(lr, pf->last_random, 32) == 0 ? MLH_OK : MLH_ERR_VERIFY;"
INDEX = "if (pf->query_indices && pf->query_indices[q] != index) return MLH_ERR_VERIFY;"
POLYS = "if (!all_canonical(pf->sumcheck_polys, 2ull * n_vars)) return MLH_ERR_VERIFY;"
BATCH_PATH = ("if (!verify_path_len(rec, 32ull * m, rec + 32ull * m, L - 1, pf->batch_commitment, index))\n"
              "      return MLH_ERR_VERIFY;")

# name -> (exact source text, replacement, expected count, which occurrence (None: all),
#          the kinds of corpus members that reach the check)
MUTANTS = {
    "K1": ("if (!verify_path(val, val + 32, depth, commitments + 32 * t, cur_idx)) return false;", "",
           1, None, ("fri", "pcs", "batched_fri", "batched_pcs")),
    "K2": ("    if (nv != folded) return false;", "", 1, None, ("fri", "batched_fri")),
    "K3": ("if (t + 1 == ntrees) return folded == last;", "if (t + 1 == ntrees) return true;", 1, None,
           ("fri", "batched_fri")),
    "K4F": (LAST_RANDOM, "return MLH_OK;", 2, 0, ("fri", "pcs")),
    "K4B": (LAST_RANDOM, "return MLH_OK;", 2, 1, ("batched_fri", "batched_pcs")),
    "K5F": (INDEX, "", 2, 0, ("fri", "pcs")),
    "K5B": (INDEX, "", 2, 1, ("batched_fri", "batched_pcs")),
    "K6P": ("if (h_mul(delta, h_load(fp->last_elem)) != eval(c, r)) return MLH_ERR_VERIFY;", "", 1, None,
            ("pcs",)),
    "K6BP": ("if (h_mul(delta, h_load(fp->last_elem)) != val) return MLH_ERR_VERIFY;", "", 1, None,
             ("batched_pcs", "system", "phased")),
    "K7": (BATCH_PATH, "", 1, None, ("batched_fri", "batched_pcs")),
    "K8": ("      if (nv != folded) return MLH_ERR_VERIFY;", "", 1, None, ("batched_fri",)),
    "K9": ("      if (folded != last) return MLH_ERR_VERIFY;", "", 1, None, ("batched_fri",)),
    "K10": ("if (h_add(h_mul(delta, comp), lin) != claim) return MLH_ERR_VERIFY;", "", 1, None,
            ("system", "phased")),
    "K11_leaf_F": ("    if (!all_canonical(val, 2)) return false;", "", 1, None, ("fri", "pcs")),
    "K11_leaf_B": ("    if (!all_canonical(rec, 2ull * m)) return MLH_ERR_VERIFY;", "", 1, None,
                   ("batched_fri", "batched_pcs")),
    "K11_poly_P": (POLYS, "", 2, 0, ("pcs",)),
    "K11_poly_BP": (POLYS, "", 2, 1, ("batched_pcs",)),
}
# Not in the table: the two `all_canonical(pf->last_elem, 1)` lines.  A
# last_elem >= M also fails K3 / K9 / K6, which compare it raw against a
# reduced value, so that mutant is equivalent; the K11 members pin the status.


def mutate(src, name):
    text, repl, count, which, _ = MUTANTS[name]
    found = src.count(text)
    assert found == count, (
        "update the mutant table: %r occurs %d times in verify.cpp, mutant %s expects %d.  The check "
        "was moved or rewritten; point the table at its new text so it keeps its mutant."
        % (text, found, name, count))
    if which is None:
        return src.replace(text, repl)
    pos = -1
    for _ in range(which + 1):
        pos = src.index(text, pos + 1)
    return src[:pos] + repl + src[pos + len(text):]


def _build(cxx, d, name, src):
    path = os.path.join(d, name + ".cpp")
    with open(path, "w") as f:
        f.write(src)
    so = os.path.join(d, name + ".so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", so, path],
                   check=True, capture_output=True, timeout=300)
    lib = ctypes.CDLL(so)
    for fn, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, fn):
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = res, args
    return lib


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    d = str(tmp_path_factory.mktemp("mutants"))
    src = open(os.path.join(CSRC, "verify.cpp")).read()  # (its relative includes: -I csrc)
    sources = {"unmodified": src}
    for name in MUTANTS:
        sources[name] = mutate(src, name)
        assert sources[name] != src
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        futs = {name: ex.submit(_build, cxx, d, name, s) for name, s in sources.items()}
        return {name: f.result() for name, f in futs.items()}


@pytest.fixture(scope="module")
def oracle_verdicts():
    return {m.id: m.oracle() for m in FR.corpus()}


def _system_members():
    out = []
    for name in FR.SYSTEM_NAMES:
        for lie in FR.SYSTEM_LIES:
            out.append(("system", name, lie))
    for name in FR.PHASED_NAMES:
        for lie in FR.PHASED_LIES[name]:
            out.append(("phased", name, lie))
    return out


def _system_accepts(lib, kind, name, lie):
    """-> (accepted by lib, accepted by the oracle)."""
    if kind == "system":
        mo, total, _ = FR.system_forgery(name, lie)
        st, digest = system_status(lib, name, mo, total)
        oracle = FR.system_verdict(mo, total)
    else:
        mo, total, cs, _ = FR.phased_forgery(name, lie)
        st, digest = phased_status(lib, name, mo, total, cs)
        oracle = FR.system_verdict(mo, total, cs)
    assert st in (0, VERIFY) and digest == (mo["digest"] if st == 0 else mo["entry"])
    return st == 0, oracle


def test_unmodified_build_gives_the_oracle_verdicts(builds, oracle_verdicts):
    lib = builds["unmodified"]
    for m in FR.corpus():
        st = c_verdict(lib, m, indices=True)
        assert st == (0 if oracle_verdicts[m.id] else VERIFY), m.id
    for kind, name, lie in _system_members():
        got, want = _system_accepts(lib, kind, name, lie)
        assert got == want == (lie is None), (kind, name, lie)


def _disagreements(lib, name, oracle_verdicts):
    kinds = MUTANTS[name][4]
    out = [m.id for m in FR.corpus()
           if m.kind in kinds and (c_verdict(lib, m, indices=True) == 0) != oracle_verdicts[m.id]]
    for kind, sname, lie in _system_members():
        if kind in kinds:
            got, want = _system_accepts(lib, kind, sname, lie)
            if got != want:
                out.append("%s-%s-%s" % (kind, sname, lie))
    return out


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_told_apart(builds, oracle_verdicts, name):
    bad = _disagreements(builds[name], name, oracle_verdicts)
    print(name, len(bad), sorted({b.split("-", 2)[2].rstrip("0123456789_") for b in bad}))
    assert bad, "no forgery reaches the check mutant %s removes" % name
    families = {b.split("-")[0] for b in bad}
    if name == "K6BP":  # also through mlh_system_verify and each opening of the phased verifier
        assert {"system-pythagorean-other_trace", "system-lin1-other_trace", "phased-quad3-other_trace_1",
                "phased-quad3-other_trace_2"} <= set(bad)
    if name == "K10":
        assert {"system", "phased"} <= families
    if name in ("K1", "K7"):  # the corpus is not Merkle-blind
        assert all("wrong_root" in b for b in bad)


def test_table_guard_names_the_remedy():
    src = open(os.path.join(CSRC, "verify.cpp")).read().replace(MUTANTS["K3"][0], "return folded == last_;")
    with pytest.raises(AssertionError, match="update the mutant table"):
        mutate(src, "K3")
