"""Random constraint programs and fill programs (tests/program_fuzz.py) on the
host: the compiler (_emit_outputs through compile_program / compile_shifted /
compile_fill) and the two host interpreters (mlh_cs_program_evaluate,
mlh_fill_program_evaluate) against the generators' own references, the
decoder's degree and inverse rules against the generators' own books, what the
committed tables cover, and the decoders, interpreters and image builders of
csrc/cs_program.hpp under ASan / UBSan over mutants of the tables' programs
(tests/fuzz/program_decode_asan.cpp, a stand-alone program).  CPU only."""
import os
import re
import shutil
import struct
import subprocess

import pytest

import program_fuzz as PF
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS

M = PF.M
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(1000, 1300)  # beside the tables' entries


def _ids(table):
    return ["%s%d" % (e["kind"], e["seed"]) for e in table]


def _rejected(make, wire):
    with pytest.raises(_lib.MlhError):
        make(wire)


# ---- host interpreters and compiler ------------------------------------------------

def _check_cs(case, tag):
    prog = CS.Program(case.wire)
    W = prog.width
    assert (W, prog.degree, prog.n_constraints, prog.n_randoms) == (
        case.width + len(case.shifts), case.degree, case.n_constraints, case.n_randoms)
    rows = PF.matrix("cpu %s" % tag, 8, W)
    rnd = PF.elements("cpu rnd %s" % tag, case.n_randoms)
    mask = PF.elements("cpu mask %s" % tag, case.n_constraints)
    for i in range(8):
        row = rows[i * W:(i + 1) * W]
        assert prog.evaluate(row, rnd, mask) == case.composition(row, rnd, mask), (tag, i)
    # one constraint at a time: a wrong output cannot hide behind the mask
    for c in range(min(case.n_constraints, 12)):
        unit = [int(k == c) for k in range(case.n_constraints)]
        assert prog.evaluate(rows[:W], rnd, unit) == case.fns[c](rows[:W], rnd) % M, (tag, c)
    return prog


def _check_fill(case, tag):
    prog = CS.FillProgram(case.wire)
    W = case.width
    assert (prog.width, prog.n_randoms, prog.n_inverses) == (W, case.n_randoms, case.n_inv)
    assert prog.output_mask == sum(1 << c for c, _ in case.outputs)
    rnd = case.randoms()
    m = case.matrix(3, 2, 4)  # 8 rows, zero INV operands among them
    for i in range(8):
        row = m[i * W:(i + 1) * W]
        assert prog.evaluate(row, rnd) == case.fill_row(row, rnd), (tag, i)
    return prog


@pytest.mark.parametrize("entry", PF.CS_TABLE, ids=_ids(PF.CS_TABLE))
def test_table_constraint_program_on_the_host(entry):
    case = PF.cs_case(entry)
    prog = _check_cs(case, case.name)
    assert case.width == entry["width"]
    assert prog.launch_info(entry["log_height"])[0] == entry["threads"]
    if not entry["small"]:  # two blocks, four row pairs per thread
        assert entry["log_height"] == {64: 10, 128: 11, 256: 12}[entry["threads"]]
        assert prog.launch_info(entry["log_height"]) == (entry["threads"], 2)
    else:
        assert entry["log_height"] <= 7


@pytest.mark.parametrize("entry", PF.FILL_TABLE, ids=_ids(PF.FILL_TABLE))
def test_table_fill_program_on_the_host(entry):
    case = PF.fill_table_case(entry)
    prog = _check_fill(case, case.name)
    assert (case.width, case.n_inv) == (entry["width"], entry["n_inv"])
    B, K, blocks = prog.launch_info(entry["log_height"])
    assert (B, K, blocks) == (entry["threads"], 1, 1) and 1 << entry["log_height"] == B
    assert bool(entry["shapes"]) == bool(case.n_inv)
    if case.n_inv:
        (Ba, Ka, La), (Bb, Kb, Lb) = entry["shapes"]
        assert Ka == 16 and 1 << La < Ba * 16       # lanes without a row
        assert Kb > 1 and 1 << Lb >= 2 * Bb * Kb    # more than one chunk
        assert max(La, Lb) <= 13


@pytest.mark.parametrize("gen", [PF.expr_case, PF.instr_case], ids=["expr", "instr"])
def test_random_constraint_programs_on_the_host(gen):
    for seed in SEEDS:
        _check_cs(gen(seed), "%s %d" % (gen.__name__, seed))


@pytest.mark.parametrize("level", ["expr", "instr"])
def test_random_fill_programs_on_the_host(level):
    for seed in SEEDS:
        _check_fill(PF.fill_case(seed, level), "fill %s %d" % (level, seed))


def test_compile_shifted_random_trees():
    """The extended row's columns width + k are the nxt columns in order of
    first appearance (left to right through the constraints)."""
    with_shifts = 0
    for seed in SEEDS:
        case = PF.expr_case(seed, width=1 + seed % 16, nxt=True)
        assert case.got_shifts == case.shifts, seed
        with_shifts += len(case.shifts) > 1
        _check_cs(case, "nxt %d" % seed)
    assert with_shifts >= 50
    with pytest.raises(ValueError):  # 33 columns with the shifted one
        CS.compile_shifted([CS.nxt(0) * CS.var(1)], 32, 0, 2)


# ---- decoder rules from the generators' books ---------------------------------------

def test_declared_degree_against_the_formal_degree():
    n = 0
    for case in [PF.cs_case(e) for e in PF.CS_TABLE] + [PF.instr_case(s) for s in SEEDS] + \
            [PF.expr_case(s) for s in SEEDS]:
        if case.level == "instr":
            wire = lambda d, case=case: PF.cs_wire_with_degree(case, d)
        else:
            wire = lambda d, case=case: CS.compile_program(case.exprs, case.width, case.n_randoms, d)
        assert 1 <= case.formal <= case.degree <= 7
        _rejected(CS.Program, wire(case.formal - 1))
        for d in range(case.formal, 8):
            assert CS.Program(wire(d)).degree == d
        _rejected(CS.Program, wire(8))
        n += 1
    assert n >= 600


def test_inverse_of_a_tainted_value_and_the_17th_inverse():
    tainted = untainted = full = 0
    cases = [PF.fill_table_case(e) for e in PF.FILL_TABLE if e["kind"] == "instr"]
    for case in cases + [PF.fill_instr_case(s) for s in SEEDS]:
        CS.FillProgram(case.wire)
        for t in range(case.n_temps):
            inv = [(PF.INV, 0, (PF.TEMP, t), (0, 0))]
            if case.n_inv == 16:
                continue
            if any(i[1] == t for i in case.instrs) and case.taint[t]:
                _rejected(CS.FillProgram, PF.fill_wire_with(case, inv))
                tainted += 1
            elif any(i[1] == t for i in case.instrs):
                assert CS.FillProgram(PF.fill_wire_with(case, inv)).n_inverses == case.n_inv + 1
                untainted += 1
        more = [(PF.INV, 0, (PF.COL, 0), (0, 0))]
        if case.n_inv == 16:
            _rejected(CS.FillProgram, PF.fill_wire_with(case, more))
            full += 1
        else:
            assert CS.FillProgram(PF.fill_wire_with(case, more)).n_inverses == case.n_inv + 1
    assert tainted >= 100 and untainted >= 100 and full >= 20
    # compile_fill: 16 inverses compile, a nested one does not
    assert CS.FillProgram(PF.fill_expr_case(5, n_inv=16).wire).n_inverses == 16
    with pytest.raises(ValueError):
        CS.compile_fill({0: CS.inv(CS.var(0) + CS.inv(CS.var(1)))}, 2, 0)
    with pytest.raises(ValueError):
        CS.compile_fill({0: sum((CS.inv(CS.var(0) + k) for k in range(17)), CS.const(0))}, 1, 0)


# ---- what the tables cover ------------------------------------------------------------

def _walk_carries(threads, W, nrows):
    """Does some thread's CsWalk::next() carry while it stages nrows x W elements?"""
    scol = threads % W
    for tid in range(threads):
        col = tid % W
        for _ in range(tid, nrows * W, threads):  # next() after every element
            col += scol
            if col >= W:
                return True
    return False


def test_constraint_table_coverage():
    entries = PF.CS_TABLE
    cases = [PF.cs_case(e) for e in entries]
    assert len(entries) >= 30
    assert sum(e["kind"] == "expr" for e in entries) >= 18
    assert sum(e["kind"] == "instr" for e in entries) >= 12
    assert len({(e["kind"], e["seed"]) for e in entries}) == len(entries)
    for threads in (256, 128, 64):
        assert sum(e["threads"] == threads and not e["small"] for e in entries) >= 3, threads
    assert {c.degree for c in cases} == set(range(1, 8))
    assert sum(c.degree > c.formal for c in cases) >= 3
    assert {1, 32} <= {c.width for c in cases}
    carrying = {c.width for c, e in zip(cases, entries) if not e["small"]
                and _walk_carries(e["threads"], c.width, min(e["threads"], 1 << (e["log_height"] - 1)))}
    assert len(carrying) >= 4, carrying
    counts = {c.n_constraints for c in cases}
    assert 1 in counts and 256 in counts
    assert any(n >= 5 and n & (n - 1) for n in counts)
    assert sum(c.shared > 0 for c in cases) >= 3  # trees that are DAGs
    heads = [struct.unpack("<7I", c.wire[:28]) for c in cases]
    assert any(h[1] == 64 and h[2] == 64 and h[5] > 1 for h in heads)  # mask indices above 128
    assert any(h[3] == 32 for h in heads)
    assert any(h[4] == 4096 and e["log_height"] <= 7 for h, e in zip(heads, entries))
    # a third of the cases take the sum-column path; bit 0, bit W - 1, all columns
    sums = [(PF.sum_mask(e, c.width), c.width) for c, e in zip(cases, entries) if e["sums"]]
    assert 3 * len(sums) >= len(entries) and all(m for m, _ in sums)
    assert any(m & 1 for m, _ in sums) and any(m >> (w - 1) for m, w in sums)
    assert any(m == (1 << w) - 1 and w > 1 for m, w in sums)
    assert any(m & (m - 1) and m != (1 << w) - 1 for m, w in sums)
    # the instruction level: every operand form
    instr = [c for c in cases if c.level == "instr"]
    feats = [PF.code_features(c.instrs, c.outs, c.n_temps) for c in instr]
    triples = set().union(*(f["triples"] for f in feats))
    want = {(op, k, pos) for op in (PF.ADD, PF.SUB, PF.MUL) for k in range(4) for pos in "ab"}
    want |= {(PF.NEG, k, "a") for k in range(4)}
    assert triples == want
    assert {o[0] for c in instr for o in c.outs} == {PF.COL, PF.RAND, PF.CONST, PF.TEMP}
    for key in ("dst_a", "dst_b", "dst_ab", "redegree", "dead"):
        assert any(f[key] for f in feats), key
    uniform = lambda o: o[0] in (PF.RAND, PF.CONST)
    assert any(op != PF.NEG and uniform(a) and uniform(b) and a[0] != b[0]
               for c in instr for op, _, a, b in c.instrs)
    assert any(op == PF.NEG and uniform(a) for c in instr for op, _, a, _ in c.instrs)
    # the 32-temp program writes all of them, the 64-entry pools are read to their ends
    big = next(c for c in instr if c.n_temps == 32)
    assert {i[1] for i in big.instrs} == set(range(32))
    pools = next(c for c in instr if len(c.consts) == 64 and c.n_randoms == 64)
    used = {o for _, _, a, b in pools.instrs for o in (a, b)} | set(pools.outs)
    assert {(PF.RAND, 63), (PF.CONST, 63)} <= used


def test_fill_table_coverage():
    entries = PF.FILL_TABLE
    cases = [PF.fill_table_case(e) for e in entries]
    assert len(entries) >= 24 and len({(e["kind"], e["seed"]) for e in entries}) == len(entries)
    assert sum(e["kind"] == "expr" for e in entries) >= 8
    assert sum(e["kind"] == "instr" for e in entries) >= 8
    for threads in (256, 128, 64):
        assert sum(e["threads"] == threads for e in entries) >= 2, threads
    assert {0, 1, 2, 5, 16} <= {c.n_inv for c in cases}
    assert any(c.n_inv == 16 and e["threads"] in (64, 128) for c, e in zip(cases, entries))
    assert {1, 32} <= {c.width for c in cases}
    instr = [c for c in cases if c.level == "instr"]
    feats = [PF.code_features(c.instrs, [(k, i) for _, k, i in c.outs], c.n_temps) for c in instr]
    assert set().union(*(f["inv_kinds"] for f in feats)) == {PF.COL, PF.RAND, PF.CONST, PF.TEMP}
    assert any(f["n_inv"] > 2 and len(f["inv_kinds"]) == 4 for f in feats)
    assert any(f["inv_dst_a"] for f in feats)
    assert any(f["taint_cycle"] for f in feats)
    assert any(k != PF.TEMP for c in instr for _, k, _ in c.outs)  # a bare operand as an output
    assert any(c.consts[a[1]] == 0 for c in instr for op, _, a, _ in c.instrs
               if op == PF.INV and a[0] == PF.CONST)
    # an output column that the program reads
    assert any((PF.COL, col) in {o for _, _, a, b in c.instrs for o in (a, b)}
               for c in instr for col, _, _ in c.outs)
    # the zero placements reach every table entry with a row-dependent INV
    for c, e in zip(cases, entries):
        for B, K, L in e["shapes"]:
            m, rnd, W = c.matrix(L, B, K), c.randoms(), c.width
            rows = [(i, v % c.n_inv) for i, v in c.zero_rows(L, B, K)]
            assert ((1 << L) - 1) in [i for i, _ in rows]
            hit = [c.zeros[v][1](m[i * W:(i + 1) * W], rnd) == 0 for i, v in rows
                   if c.zeros[v][0] is not None]
            assert all(hit), (c.name, B, K, L)
            assert hit or all(col is None for col, _ in c.zeros), (c.name, B, K, L)


# ---- the decoders under ASan / UBSan ---------------------------------------------------

def test_program_decoders_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "program_decode_asan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "fuzz", "program_decode_asan.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    progs = [(0, PF.cs_case(e).wire) for e in PF.CS_TABLE]
    progs += [(1, PF.fill_table_case(e).wire) for e in PF.FILL_TABLE]
    blob = struct.pack("<I", len(progs)) + b"".join(
        struct.pack("<BI", k, len(w)) + w for k, w in progs)
    seed = tmp_path / "programs.bin"
    seed.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(seed), "40000"], capture_output=True, text=True, timeout=600,
                       env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"program decode ok: accepted (\d+) rejected (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0
