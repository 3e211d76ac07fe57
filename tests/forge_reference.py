"""Cheating provers and a check-by-check verifier, for
tests/test_verifier_forgeries_*.py and tests/test_verifier_mutants_cpu.py.
Plain Python over oracle/ (and the system models tests/system_reference.py,
tests/phased_reference.py); no libmlhip arithmetic.

A forger is the oracle's prover with one controlled lie: the transcript, the
Merkle trees and the openings stay consistent with what was committed, so the
proof passes every check but the one the lie is aimed at.  lie=None gives the
oracle's own proof, byte for byte.  A lie is a tuple (family, argument...):

  shift_layer t        layer t >= 1 is the honest fold plus 1 (still an RS code);
                       batched: layer 0 is the batch layer, layer 1 the first
                       inner tree
  wrong_challenge k    step k folds with r + 1, the transcript drew r
  last_elem            last_elem + 1, absorbed as such
  batch_column j       code j of the batch layer committed plus 1, the inner
                       layers fold the fingerprints of the unshifted codes
  wrong_fingerprint    the fingerprints use fr + 1
  wrong_claim [j]      output (+1) / outputs[j] (+1) claimed, absorbed, the
                       sumcheck runs from it
  swapped_outputs i j  two distinct outputs exchanged in the claim
  wrong_poly k         coefficient c1 of round k plus 1, later rounds follow it
  other_polynomial     the code commits to g != f, sumcheck and claim are f's
  wrong_root t         the root of layer t is published and absorbed as another
                       digest; the openings come from the real tree
  wrong_index d        every opening taken at (drawn + d) mod n, valid paths
  wrong_directions     honest openings whose tree-0 directions spell index ^ 1
                       (what a decoder would hand over as query_indices)
  stale_last_random    last_random taken before the last index absorb
  noncanonical where   leaf / last_elem / poly: an element x < 2^128 - M stored
                       as x + M, trees and transcript over those bytes

explain() replays the verifier without stopping and names every failing check:

  K1(t) Merkle path of tree t (hashed in the order the drawn index dictates)
  K2(t) fold t -> t+1          K3  last fold against last_elem
  K4    last_random            K5  the path's directions spell another index
  K6    final delta check of PCS / batched PCS
  K7    batch path             K8  batch -> inner boundary
  K9    batch fold against last_elem (no inner tree)
  K10   final check of the constraint sumcheck
  K11   non-canonical element
Batched proofs number their inner trees from 0 in K1 / K2.
"""
import functools
import hashlib
import random

import phased_reference as PR
import system_reference as S
from oracle import batched as OB
from oracle import field as F
from oracle import fri as OF
from oracle import merkle as MK
from oracle import pcs as OP
from oracle import transcript as OT
from oracle.ntt import bit_reverse_permutation
from oracle.polynomials import interpolate, to_coefficient, uni_evaluate
from oracle.sumcheck import SumcheckTables, delta_evaluate, to_polynomial

M = F.M
NC = 2**128 - M  # x < NC: x + M still fits 16 bytes (45 * 2^40 - 1)
NQ = OF.NUM_QUERIES


def _is(lie, name, *args):
    return lie is not None and lie[0] == name and tuple(lie[1:1 + len(args)]) == args


def _bump(x):
    return (x + 1) % M


def _noncanonical(x):
    assert x < NC, "the targeted value must be below 2^128 - M"
    return x + M


def rand_vals(seed, n):
    r = random.Random(seed)
    return [r.randrange(M) for _ in range(n)]


# ---- the shared steps ---------------------------------------------------------

def _last_element(nxt, tr, lie):
    assert all(x == nxt[0] for x in nxt), "not an RS code"
    last = nxt[0]
    if _is(lie, "last_elem"):
        last = _bump(last)
    if _is(lie, "noncanonical", "last_elem"):
        last = _noncanonical(last)
    tr.absorb(F.to_bytes(last))
    return last


def _publish(tree, tr, lie, layer):
    """Absorbs the tree's root; wrong_root(layer): another digest takes its
    place in the proof and in the transcript, the paths stay the real tree's."""
    if _is(lie, "wrong_root", layer):
        tree.layers[-1] = [hashlib.sha256(tree.root()).digest()]
    tr.absorb(tree.root())


def _fold_step(fri, gen_pows, k, r, tr, lie, layer):
    """FriProverData.fold_step (oracle/fri.py); `layer` numbers the layer it
    creates (the committed code is layer 0)."""
    last = fri.merkle_trees[-1].pairs
    half_n = len(last)
    assert 2 * half_n > 1 << OF.LOG_BLOWUP
    nxt = OF.fold_layer(last, gen_pows, k, _bump(r) if _is(lie, "wrong_challenge", k) else r)
    if half_n == 1 << OF.LOG_BLOWUP:
        fri.last_element = _last_element(nxt, tr, lie)
        return
    if _is(lie, "shift_layer", layer):
        nxt = [_bump(x) for x in nxt]
    tree = OF.commit_rs_code(nxt)
    fri.merkle_trees.append(tree)
    _publish(tree, tr, lie, layer)


def _batched_fold_step(pd, pairs, gen_pows, r, tr, lie):
    """BatchedFriProverData.batched_fold_step (oracle/batched.py) on the
    fingerprints of `pairs` (the committed ones unless a column lies)."""
    half_n = len(pairs[0])
    fr = _bump(pd.fingerprint_r) if _is(lie, "wrong_fingerprint") else pd.fingerprint_r
    fp = [(OB.fingerprint(fr, [p[i][0] for p in pairs]), OB.fingerprint(fr, [p[i][1] for p in pairs]))
          for i in range(half_n)]
    nxt = OF.fold_layer(fp, gen_pows, 0, _bump(r) if _is(lie, "wrong_challenge", 0) else r)
    if half_n == 1 << OF.LOG_BLOWUP:
        pd.fri_data.last_element = _last_element(nxt, tr, lie)
        return
    if _is(lie, "shift_layer", 1):
        nxt = [_bump(x) for x in nxt]
    tree = OF.commit_rs_code(nxt)
    pd.fri_data.merkle_trees.append(tree)
    _publish(tree, tr, lie, 1)


def _flip_first_direction(path):
    (sib, d) = path[0]
    return [(sib, d ^ 1)] + list(path[1:])


def _queries(open_at, tr, domain, lie, batched):
    """The query loop of every prove(): -> (queries, last_random)."""
    n = domain // 2
    d = lie[1] if _is(lie, "wrong_index") else 0
    queries, stale, drawn = [], None, []
    for _ in range(NQ):
        idx = OF.query_index(tr, domain)
        drawn.append(idx)
        q = open_at((idx + d) % n)
        if _is(lie, "wrong_directions"):
            if batched:
                (value, path), inner = q
                q = ((value, _flip_first_direction(path)), inner)
            else:
                q = [(q[0][0], _flip_first_direction(q[0][1]))] + list(q[1:])
        queries.append(q)
        stale = tr.random()
        tr.absorb(idx.to_bytes(8, "little"))
    if _is(lie, "noncanonical", "leaf"):
        assert 0 in drawn, "no query reads the non-canonical leaf"
    return queries, stale if _is(lie, "stale_last_random") else tr.random()


def _round(tables, prev, tr, lie, k):
    """SumcheckTables.compute_sumcheck_polynomial (oracle/sumcheck.py), degree 2."""
    evals = [0, tables.partial_sum(F.from_i64(1)), tables.partial_sum(F.from_i64(2))]
    evals[0] = (prev - evals[1]) % M
    nz = list(interpolate(evals)[1:])
    if _is(lie, "wrong_poly", k):
        nz[0] = _bump(nz[0])
    if _is(lie, "noncanonical", "poly") and k == 0:
        nz[1] = _noncanonical(nz[1])
    for c in nz:
        tr.absorb(F.to_bytes(c))
    r = tr.next_challenge()
    new_prev = uni_evaluate(to_polynomial([c % M for c in nz], prev), r) % M  # as the verifier
    tables.fold(r)
    return tuple(nz), r, new_prev


def _fri_init(code, tr, lie):
    """FriProverData.init (oracle/fri.py)."""
    tree = OF.commit_rs_code(code)
    _publish(tree, tr, lie, 0)
    return OF.FriProverData([tree], None)


def _rs_code(evals, gen):
    c = to_coefficient(evals)
    bit_reverse_permutation(c)
    return OF.reed_solomon(c, gen)


def _other(evals):
    return [_bump(evals[0])] + list(evals[1:])


# ---- the four forgers ---------------------------------------------------------

def forge_fri(code, gen_pows, tr, lie=None):
    """FriProof.prove with `lie`."""
    code = list(code)
    if _is(lie, "noncanonical", "leaf"):
        code[0] = _noncanonical(code[0])
    fri = _fri_init(code, tr, lie)
    steps = (len(code).bit_length() - 1) - OF.LOG_BLOWUP
    for k in range(steps):
        _fold_step(fri, gen_pows, k, tr.next_challenge(), tr, lie, k + 1)
    queries, last_random = _queries(fri.open_query_at, tr, len(code), lie, False)
    return OF.FriProof(fri.fold_roots(), queries, fri.last_element, last_random)


def forge_pcs(inputs, output, evals, tr, lie=None):
    """PCSProof.prove with `lie`; the proof carries the claimed output."""
    log_domain = (len(evals).bit_length() - 1) + OF.LOG_BLOWUP
    gen_pows = F.pow_2_generator_powers(log_domain)
    code = _rs_code(_other(evals) if _is(lie, "other_polynomial") else evals, gen_pows[1])
    if _is(lie, "noncanonical", "leaf"):
        code[0] = _noncanonical(code[0])
    fri = _fri_init(code, tr, lie)
    tables = SumcheckTables.build_tables_for_pcs(inputs, evals)
    claim = _bump(output) if _is(lie, "wrong_claim") else output
    prev, polys = claim, []
    for k in range(log_domain - OF.LOG_BLOWUP):
        nz, r, prev = _round(tables, prev, tr, lie, k)
        polys.append(nz)
        _fold_step(fri, gen_pows, k, r, tr, lie, k + 1)
    queries, last_random = _queries(fri.open_query_at, tr, 1 << log_domain, lie, False)
    fp = OF.FriProof(fri.fold_roots(), queries, fri.last_element, last_random)
    return OP.PCSProof(fp, polys, list(inputs), claim)


def _batched_init(codes, tr, lie):
    codes = [list(c) for c in codes]
    if _is(lie, "noncanonical", "leaf"):
        codes[-1][0] = _noncanonical(codes[-1][0])
    committed = codes
    if _is(lie, "batch_column"):
        committed = [[_bump(x) for x in c] if j == lie[1] else c for j, c in enumerate(codes)]
    h = len(codes[0]) // 2

    def pairs_of(cs):
        return [[(c[i], c[i + h]) for i in range(h)] for c in cs]

    # BatchedFriProverData.init (oracle/batched.py)
    layer = MK.Merkle.batch_commit([[OF.pair_bytes(a, b) for a, b in p] for p in pairs_of(committed)])
    layer.pairs = pairs_of(committed)
    _publish(layer, tr, lie, 0)
    fr = tr.next_challenge()
    tr.absorb(F.to_bytes(fr))
    return OB.BatchedFriProverData(layer, fr, OF.FriProverData([], None)), pairs_of(codes)


def forge_batched_fri(codes, gen_pows, tr, lie=None):
    """BatchedFriProof.prove with `lie`."""
    pd, pairs = _batched_init(codes, tr, lie)
    steps = (len(codes[0]).bit_length() - 1) - OF.LOG_BLOWUP
    _batched_fold_step(pd, pairs, gen_pows, tr.next_challenge(), tr, lie)
    for k in range(1, steps):
        _fold_step(pd.fri_data, gen_pows, k, tr.next_challenge(), tr, lie, k + 1)
    queries, last_random = _queries(pd.open_query_at, tr, len(codes[0]), lie, True)
    return OB.BatchedFriProof(pd.batch_layer.root(), pd.fri_data.fold_roots(), queries,
                              pd.fri_data.last_element, last_random)


def forge_batched_pcs(inputs, outputs, polys, tr, lie=None):
    """BatchedPCSProof.prove with `lie`; the proof carries the claimed outputs."""
    log_domain = (len(polys[0]).bit_length() - 1) + OF.LOG_BLOWUP
    gen_pows = F.pow_2_generator_powers(log_domain)
    codes = [_rs_code(_other(p) if j == 0 and _is(lie, "other_polynomial") else p, gen_pows[1])
             for j, p in enumerate(polys)]
    claimed = list(outputs)
    if _is(lie, "wrong_claim"):
        claimed[lie[1]] = _bump(claimed[lie[1]])
    if _is(lie, "swapped_outputs"):
        i, j = lie[1], lie[2]
        assert claimed[i] != claimed[j]
        claimed[i], claimed[j] = claimed[j], claimed[i]
    for x in inputs:
        tr.absorb(F.to_bytes(x))
    for y in claimed:
        tr.absorb(F.to_bytes(y))
    pd, pairs = _batched_init(codes, tr, lie)
    fr = pd.fingerprint_r
    fp = [OB.fingerprint(fr, [p[i] for p in polys]) for i in range(len(polys[0]))]
    tables = SumcheckTables.build_tables_for_pcs(inputs, fp)
    prev, sc = OB.fingerprint(fr, claimed), []
    for k in range(log_domain - OF.LOG_BLOWUP):
        nz, r, prev = _round(tables, prev, tr, lie, k)
        sc.append(nz)
        if k == 0:
            _batched_fold_step(pd, pairs, gen_pows, r, tr, lie)
        else:
            _fold_step(pd.fri_data, gen_pows, k, r, tr, lie, k + 1)
    queries, last_random = _queries(pd.open_query_at, tr, 1 << log_domain, lie, True)
    proof = OB.BatchedFriProof(pd.batch_layer.root(), pd.fri_data.fold_roots(), queries,
                               pd.fri_data.last_element, last_random)
    return OB.BatchedPCSProof(proof, sc, list(inputs), claimed)


def proof_bytes(p):
    """Everything a proof holds, flat (directions included), for equality."""
    if isinstance(p, (OP.PCSProof, OB.BatchedPCSProof)):
        out = getattr(p, "outputs", None) or [p.output]
        return (proof_bytes(p.fri_proof) + b"".join(F.to_bytes(c) for s in p.sumcheck_polynomials for c in s)
                + b"".join(F.to_bytes(x) for x in list(p.inputs) + list(out)))

    def paths(ps):
        return b"".join(v + b"".join(s + bytes([d]) for s, d in path) for v, path in ps)

    raw = b"".join(p.commitments) + F.to_bytes(p.last_elem) + p.last_random
    if isinstance(p, OB.BatchedFriProof):
        raw += p.batch_commitment
        for (col, bpath), inner in p.queries:
            raw += b"".join(col) + b"".join(s + bytes([d]) for s, d in bpath) + paths(inner)
    else:
        for q in p.queries:
            raw += paths(q)
    return raw


def spelled_index(path):
    """The index a path's directions spell (merkle_tree/mod.rs:216-253)."""
    return sum(1 << i for i, (_, d) in enumerate(path) if d == MK.LEFT)


def opened_indices(p):
    """What a decoder derives as query_indices: the tree-0 directions."""
    fp = getattr(p, "fri_proof", p)
    if isinstance(fp, OB.BatchedFriProof):
        return [spelled_index(bpath) for (_, bpath), _ in fp.queries]
    return [spelled_index(q[0][1]) for q in fp.queries]


# ---- flat records (the C layout) -> oracle proofs ---------------------------------

def _path(sibs, index):
    return [(s, MK.LEFT if (index >> level) & 1 else MK.RIGHT) for level, s in enumerate(sibs)]


def _chain_from_flat(raw, off, depth0, ntrees, index):
    paths, n = [], 1 << depth0
    for t in range(ntrees):
        depth = depth0 - t
        sibs = [raw[off + 32 * (1 + i):off + 32 * (2 + i)] for i in range(depth)]
        paths.append((raw[off:off + 32], _path(sibs, index)))
        off += 32 * (1 + depth)
        n //= 2
        index %= max(n, 1)
    return paths, off


def fri_from_flat(commitments, raw, indices, last_elem, last_random):
    """A FriProof from the flat query records of mlhip.h; the directions are
    those `indices` (the prover's query_indices) spell."""
    T = len(commitments)
    qb = len(raw) // len(indices)
    queries = [_chain_from_flat(raw, q * qb, T, T, idx)[0] for q, idx in enumerate(indices)]
    return OF.FriProof(list(commitments), queries, last_elem, last_random)


def batched_from_flat(batch_commitment, commitments, m, raw, indices, last_elem, last_random):
    """A BatchedFriProof from the flat batched records of mlhip.h."""
    T = len(commitments)
    depth = T + 1  # leaves of the batch layer: 2^(log_code - 1)
    qb = len(raw) // len(indices)
    queries = []
    for q, idx in enumerate(indices):
        off = q * qb
        col = [raw[off + 32 * j:off + 32 * j + 32] for j in range(m)]
        off += 32 * m
        sibs = [raw[off + 32 * i:off + 32 * i + 32] for i in range(depth)]
        off += 32 * depth
        inner, _ = _chain_from_flat(raw, off, T, T, idx % (1 << T))
        queries.append(((col, _path(sibs, idx)), inner))
    return OB.BatchedFriProof(batch_commitment, list(commitments), queries, last_elem, last_random)


# ---- explain ------------------------------------------------------------------

def _hash_ok(value, path, root, index):
    h = hashlib.sha256(value).digest()
    for level, (sib, _) in enumerate(path):
        h = MK.hash_node(sib, h) if (index >> level) & 1 else MK.hash_node(h, sib)
    return h == root


def _elem(raw, out):
    v = F.from_bytes(raw)
    if v >= M:
        out.add("K11")
    return v % M


def _fold(v, mv, gp, r):
    return (F.div(v + mv, 2) + r * F.div(v - mv, F.mul(2, gp))) % M


def _chain(paths, commitments, last, n, index, gen, rs, out):
    """verify_query (oracle/fri.py) without stopping."""
    cur_n, cur_idx, cur_gen = n, index, gen
    for i, (value, path) in enumerate(paths):
        if not _hash_ok(value, path, commitments[i], cur_idx):
            out.add("K1(%d)" % i)
        if spelled_index(path) != cur_idx:
            out.add("K5")
        folded = _fold(_elem(value[:16], out), _elem(value[16:32], out), F.fpow(cur_gen, cur_idx), rs[i])
        if i == len(paths) - 1:
            if folded != last % M:
                out.add("K3")
            return
        nxt_idx = cur_idx % (cur_n // 2)
        nv = paths[i + 1][0]
        if F.from_bytes(nv[:16] if nxt_idx == cur_idx else nv[16:32]) % M != folded:
            out.add("K2(%d)" % i)
        cur_gen, cur_n, cur_idx = F.mul(cur_gen, cur_gen), cur_n // 2, nxt_idx


def _explain_fri_queries(fp, tr, rs, out):
    log_domain = len(fp.commitments) + OF.LOG_BLOWUP
    gen = F.pow_2_generator(log_domain)
    if fp.last_elem >= M:
        out.add("K11")
    for q in fp.queries:
        idx = OF.query_index(tr, 1 << log_domain)
        tr.absorb(idx.to_bytes(8, "little"))
        _chain(q, fp.commitments, fp.last_elem, (1 << log_domain) // 2, idx, gen, rs, out)
    if fp.last_random != tr.random():
        out.add("K4")


def _explain_batched_queries(fp, tr, rs, fr, out):
    log_domain = len(fp.commitments) + 1 + OF.LOG_BLOWUP
    gen, n = F.pow_2_generator(log_domain), (1 << log_domain) // 2
    if fp.last_elem >= M:
        out.add("K11")
    for (value, path), inner in fp.queries:
        idx = OF.query_index(tr, 1 << log_domain)
        tr.absorb(idx.to_bytes(8, "little"))
        if not _hash_ok(b"".join(value), path, fp.batch_commitment, idx):
            out.add("K7")
        if spelled_index(path) != idx:
            out.add("K5")
        v = OB.fingerprint(fr, [_elem(p[:16], out) for p in value])
        mv = OB.fingerprint(fr, [_elem(p[16:32], out) for p in value])
        folded = _fold(v, mv, F.fpow(gen, idx), rs[0])
        if not inner:
            if folded != fp.last_elem % M:
                out.add("K9")
            continue
        nxt_idx = idx % (n // 2)
        nv = inner[0][0]
        if F.from_bytes(nv[:16] if nxt_idx == idx else nv[16:32]) % M != folded:
            out.add("K8")
        _chain(inner, fp.commitments, fp.last_elem, n // 2, nxt_idx, F.mul(gen, gen), rs[1:], out)
    if fp.last_random != tr.random():
        out.add("K4")


def _sumcheck_chain(polys, claim, rs, out):
    """The to_polynomial chain of both PCS verifiers -> the last evaluation."""
    val = claim
    for sp, r in zip(polys, rs):
        if any(c >= M for c in sp):
            out.add("K11")
        val = uni_evaluate(to_polynomial([c % M for c in sp], val), r) % M
    return val


def explain(proof, tr=None):
    """-> the set of failing checks.  tr: the transcript a PCS proof is
    verified on (advanced as the verifier advances it)."""
    out = set()
    if isinstance(proof, OF.FriProof):
        tr, rs = OT.Transcript(), []
        for root in proof.commitments:
            tr.absorb(root)
            rs.append(tr.next_challenge())
        tr.absorb(F.to_bytes(proof.last_elem))
        _explain_fri_queries(proof, tr, rs, out)
    elif isinstance(proof, OB.BatchedFriProof):
        tr = OT.Transcript()
        tr.absorb(proof.batch_commitment)
        fr = tr.next_challenge()
        tr.absorb(F.to_bytes(fr))
        rs = [tr.next_challenge()]
        for c in proof.commitments:
            tr.absorb(c)
            rs.append(tr.next_challenge())
        tr.absorb(F.to_bytes(proof.last_elem))
        _explain_batched_queries(proof, tr, rs, fr, out)
    elif isinstance(proof, OP.PCSProof):
        fp, rs = proof.fri_proof, []
        for root, poly in zip(fp.commitments, proof.sumcheck_polynomials):
            tr.absorb(root)
            for c in poly:
                tr.absorb(F.to_bytes(c))
            rs.append(tr.next_challenge())
        tr.absorb(F.to_bytes(fp.last_elem))
        val = _sumcheck_chain(proof.sumcheck_polynomials, proof.output, rs, out)
        if delta_evaluate(proof.inputs, rs) * fp.last_elem % M != val:
            out.add("K6")
        _explain_fri_queries(fp, tr, rs, out)
    elif isinstance(proof, OB.BatchedPCSProof):
        fp, rs, fr = proof.fri_proof, [], 0
        for x in proof.inputs:
            tr.absorb(F.to_bytes(x))
        for y in proof.outputs:
            tr.absorb(F.to_bytes(y))
        for i, poly in enumerate(proof.sumcheck_polynomials):
            if i == 0:
                tr.absorb(fp.batch_commitment)
                fr = tr.next_challenge()
                tr.absorb(F.to_bytes(fr))
            else:
                tr.absorb(fp.commitments[i - 1])
            for c in poly:
                tr.absorb(F.to_bytes(c))
            rs.append(tr.next_challenge())
        tr.absorb(F.to_bytes(fp.last_elem))
        val = _sumcheck_chain(proof.sumcheck_polynomials, OB.fingerprint(fr, proof.outputs), rs, out)
        if delta_evaluate(proof.inputs, rs) * fp.last_elem % M != val:
            out.add("K6")
        _explain_batched_queries(fp, tr, rs, fr, out)
    else:
        raise TypeError(type(proof))
    return out


def oracle_verdict(proof, tr=None):
    """The oracle's own verify() (it stops at the first failure)."""
    if isinstance(proof, (OF.FriProof, OB.BatchedFriProof)):
        return proof.verify()
    return proof.verify(tr)


# ---- system level -------------------------------------------------------------

def _system_replay(mo, total, column_sum=None):
    """The verifier's side of the head and the constraint sumcheck of a model
    proof `mo` (system_reference / phased_reference) -> (tr, rs, K10 holds)."""
    sysm = mo["sysm"]
    phased = "root1" in mo
    tr = OT.Transcript()
    tr.absorb(mo["seed"])
    tr.absorb(mo["root1"] if phased else mo["root"])
    trace = [tr.next_challenge()] * len(sysm.challenges.trace)
    if phased and mo["root2"] is not None:
        tr.absorb(mo["root2"])
    from cs_reference import System

    vs = System(tr, sysm.constraints, sysm.degree, sysm.columns, len(trace), mo["log_height"])
    vs.challenges.trace = trace
    beta, claim = 0, total
    if phased and mo["sum_columns"]:
        tr.absorb(F.to_bytes(column_sum))
        beta = tr.next_challenge()
        claim = (total + beta * column_sum) % M
    rs, val = vs._replay(tr, mo["pols"], claim)
    lin = beta * sum(mo["output"][j] for j in mo.get("sum_columns", ())) % M
    ok = (F.mul(vs.evaluate_delta(rs), vs.evaluate_composition(mo["output"])) + lin) % M == val
    return tr, rs, ok


def _openings(mo):
    """[(BatchedPCSProof, outputs)] of a model proof, in order."""
    if "root1" not in mo:
        return [(mo["openings"][0], mo["output"])]
    P = mo["pre"]
    outs = [mo["output"][:P], mo["output"][P:]]
    return [(pr, outs[i]) for i, pr in enumerate(mo["openings"])]


def explain_system(mo, total, column_sum=None):
    """explain() of a system / phased model proof verified against `total`
    (and `column_sum`); the openings' labels carry their number: "K6@0"."""
    tr, rs, ok = _system_replay(mo, total, column_sum)
    out = set() if ok else {"K10"}
    for i, (pr, outputs) in enumerate(_openings(mo)):
        claimed = OB.BatchedPCSProof(pr.fri_proof, pr.sumcheck_polynomials, rs, list(outputs))
        out |= {"%s@%d" % (k, i) for k in explain(claimed, tr)}
    return out


def system_verdict(mo, total, column_sum=None):
    """The oracle's verdict: sumcheck.rs:91-124, then each opening's verify()."""
    tr, rs, ok = _system_replay(mo, total, column_sum)
    if not ok:
        return False
    for pr, outputs in _openings(mo):
        if not OB.BatchedPCSProof(pr.fri_proof, pr.sumcheck_polynomials, rs, list(outputs)).verify(tr):
            return False
    return True


@functools.lru_cache(maxsize=None)
def system_forgery(name, lie):
    """-> (model proof, total to verify against, expected explain())."""
    c = None if name == "pythagorean" else S.CASES[name]
    import cs_cases

    args = ((b"", cs_cases.PYTHAGOREAN_FNS, 2, 4, 0, 4, cs_cases.pythagorean_matrix()) if c is None
            else (c.seed, c.fns, c.degree, c.width, c.randoms, c.log_height, c.matrix()))
    honest = S.model(name)
    if lie is None:
        return honest, honest["total"], set()
    if lie == "wrong_total_consistent":
        t = _bump(honest["total"])
        return S.prove(*args, total=t), t, {"K10"}
    if lie == "other_trace":
        other = [_bump(v) for v in args[6]]
        mo = S.prove(*args, opening_matrix=other)  # the true sum under this root's challenges
        return mo, mo["total"], {"K6@0"}
    raise ValueError(lie)


@functools.lru_cache(maxsize=None)
def phased_forgery(name, lie):
    """-> (model proof, total, column_sum, expected explain())."""
    P, sc = PR.LAYOUTS[name]
    import cs_cases

    c = None if name == "pythagorean" else S.CASES[name]
    args = ((b"", cs_cases.PYTHAGOREAN_FNS, 2, 4, 0, 4, cs_cases.pythagorean_matrix()) if c is None
            else (c.seed, c.fns, c.degree, c.width, c.randoms, c.log_height, c.matrix()))
    honest = PR.model(name)
    tot, cs = honest["total"], honest["column_sum"]
    if lie is None:
        return honest, tot, cs, set()
    other = [_bump(v) for v in args[6]]
    if lie == "wrong_total_consistent":
        return PR.prove(*args, P, sc, total=_bump(tot)), _bump(tot), cs, {"K10"}
    if lie == "wrong_column_sum_consistent":
        return PR.prove(*args, P, sc, total=tot, column_sum=_bump(cs)), tot, _bump(cs), {"K10"}
    if lie in ("other_trace_1", "other_trace_2"):  # the true sums under these roots' challenges
        mo = PR.prove(*args, P, sc, **{"matrix" + lie[-1]: other})
        return mo, mo["total"], mo["column_sum"], {"K6@" + str(int(lie[-1]) - 1)}
    raise ValueError(lie)


# ---- the corpus ---------------------------------------------------------------

FRI_LOGS = (1, 2, 3, 5)
BATCHED_SHAPES = ((1, 1), (2, 1), (3, 2), (2, 4))
WRONG_INDEX_LABELS = ("K1", "K2", "K3", "K5", "K7", "K8", "K9")


def fold_check(k, steps, batched=False):
    """The check that sees a wrong fold at step k of `steps`."""
    if batched and k == 0:
        return "K9" if steps == 1 else "K8"
    if k == steps - 1:
        return "K3"
    return "K2(%d)" % (k - 1 if batched else k)


def small_vals(n, j=0):
    return [F.from_i64(7 * i + 3 + 100 * j) for i in range(n)]


def _index_lies(n):
    """n: leaves of tree 0.  d = 1 and d = n/2 (one lie where they coincide)."""
    return [("wrong_index", d) for d in sorted({1, n // 2} - {0})]


class Member:
    """One corpus proof.  expect: the exact explain() set; for wrong_index the
    family touches the path and the fold's twiddle of every query, so K5 and
    any of WRONG_INDEX_LABELS (kind-dependent) may be named."""

    def __init__(self, kind, shape, lie, proof, expect, start=None):
        self.kind, self.shape, self.lie, self.proof, self.expect = kind, shape, lie, proof, expect
        self.start = start  # bytes absorbed before a PCS proof
        self.id = "%s-%s-%s" % (kind, "x".join(map(str, shape)), "_".join(map(str, lie or ("honest",))))

    def transcript(self):
        tr = OT.Transcript()
        if self.start:
            tr.absorb(self.start)
        return tr

    def explain(self):
        return explain(self.proof, self.transcript())

    def oracle(self):
        return oracle_verdict(self.proof, self.transcript())

    def matches(self, got):
        if self.lie and self.lie[0] == "wrong_index":
            return "K5" in got and all(k.startswith(WRONG_INDEX_LABELS) for k in got)
        return got == self.expect


def _fri_members():
    out = []
    for ln in FRI_LOGS:
        gp = F.pow_2_generator_powers(ln + 1)
        steps = ln
        lies = [(None, None)]
        lies += [(("shift_layer", t), {fold_check(t - 1, steps)}) for t in range(1, steps)]
        lies += [(("wrong_challenge", k), {fold_check(k, steps)}) for k in range(steps)]
        lies += [(("wrong_root", t), {"K1(%d)" % t}) for t in range(steps)]
        lies += [(("last_elem",), {"K3"}), (("stale_last_random",), {"K4"}), (("wrong_directions",), {"K5"})]
        lies += [(l, None) for l in _index_lies(1 << ln)]
        for lie, expect in lies:
            code = OF.reed_solomon(rand_vals(100 + ln, 1 << ln), gp[1])
            out.append(Member("fri", (ln,), lie, forge_fri(code, gp, OT.Transcript(), lie), expect or set()))
        code = OF.reed_solomon(small_vals(1 << ln), gp[1])
        out.append(Member("fri", (ln,), ("noncanonical", "leaf"),
                          forge_fri(code, gp, OT.Transcript(), ("noncanonical", "leaf")), {"K11"}))
        code = OF.reed_solomon([5] + [0] * ((1 << ln) - 1), gp[1])
        out.append(Member("fri", (ln,), ("noncanonical", "last_elem"),
                          forge_fri(code, gp, OT.Transcript(), ("noncanonical", "last_elem")), {"K11"}))
    return out


def _mle(evals, pts):
    from oracle.polynomials import mle_evaluate

    return mle_evaluate(evals, pts)


def _pcs_members():
    out = []
    for n in FRI_LOGS:
        start = b"pcs%d" % n
        pts = rand_vals(200 + n, n)
        lies = [(None, set()), (("wrong_claim",), {"K6"}), (("other_polynomial",), {"K6"}),
                (("stale_last_random",), {"K4"}), (("wrong_directions",), {"K5"}),
                (("wrong_root", n - 1), {"K1(%d)" % (n - 1)})]
        lies += [(("wrong_poly", k), {"K6"}) for k in range(n)]
        lies += [(l, None) for l in _index_lies(1 << n)]
        for lie, expect in lies:
            ev = rand_vals(300 + n, 1 << n)
            m = Member("pcs", (n,), lie, None, expect or set(), start)
            m.proof = forge_pcs(pts, _mle(ev, pts), ev, m.transcript(), lie)
            out.append(m)
        for where, ev in (("leaf", small_vals(1 << n)), ("last_elem", [5] * (1 << n)),
                          ("poly", [5] * (1 << n))):
            m = Member("pcs", (n,), ("noncanonical", where), None, {"K11"}, start)
            m.proof = forge_pcs(pts, _mle(ev, pts), ev, m.transcript(), m.lie)
            out.append(m)
    return out


def _batched_fri_members():
    out = []
    for m_, ln in BATCHED_SHAPES:
        gp = F.pow_2_generator_powers(ln + 1)
        steps = ln
        lies = [(None, set())]
        lies += [(("shift_layer", t), {fold_check(t - 1, steps, True)}) for t in range(1, steps)]
        lies += [(("wrong_challenge", k), {fold_check(k, steps, True)}) for k in range(steps)]
        lies += [(("batch_column", j), {fold_check(0, steps, True)}) for j in range(m_)]
        lies += [(("wrong_root", t), {"K1(%d)" % (t - 1) if t else "K7"}) for t in range(steps)]
        if m_ > 1:  # one code: the fingerprint is the code, whatever fr
            lies.append((("wrong_fingerprint",), {fold_check(0, steps, True)}))
        lies += [(("last_elem",), {"K9" if steps == 1 else "K3"}), (("stale_last_random",), {"K4"}),
                 (("wrong_directions",), {"K5"})]
        lies += [(l, None) for l in _index_lies(1 << ln)]
        for lie, expect in lies:
            codes = [OF.reed_solomon(rand_vals(400 + 10 * ln + j, 1 << ln), gp[1]) for j in range(m_)]
            out.append(Member("batched_fri", (m_, ln), lie,
                              forge_batched_fri(codes, gp, OT.Transcript(), lie), expect or set()))
        codes = [OF.reed_solomon(small_vals(1 << ln, j), gp[1]) for j in range(m_)]
        out.append(Member("batched_fri", (m_, ln), ("noncanonical", "leaf"),
                          forge_batched_fri(codes, gp, OT.Transcript(), ("noncanonical", "leaf")), {"K11"}))
        if m_ == 1:  # a fingerprint of constants is small only for one code
            codes = [OF.reed_solomon([5] + [0] * ((1 << ln) - 1), gp[1])]
            out.append(Member("batched_fri", (m_, ln), ("noncanonical", "last_elem"),
                              forge_batched_fri(codes, gp, OT.Transcript(), ("noncanonical", "last_elem")),
                              {"K11"}))
    return out


def _batched_pcs_members():
    out = []
    for m_, n in BATCHED_SHAPES:
        start = b"bpcs%d_%d" % (m_, n)
        pts = rand_vals(500 + n, n)
        lies = [(None, set()), (("other_polynomial",), {"K6"}), (("stale_last_random",), {"K4"}),
                (("wrong_directions",), {"K5"}), (("wrong_root", 0), {"K7"})]
        lies += [(("wrong_claim", j), {"K6"}) for j in range(m_)]
        if m_ > 1:
            lies.append((("swapped_outputs", 0, m_ - 1), {"K6"}))
        lies += [(("wrong_poly", k), {"K6"}) for k in range(n)]
        lies += [(l, None) for l in _index_lies(1 << n)]
        for lie, expect in lies:
            polys = [rand_vals(600 + 10 * n + j, 1 << n) for j in range(m_)]
            mb = Member("batched_pcs", (m_, n), lie, None, expect or set(), start)
            mb.proof = forge_batched_pcs(pts, [_mle(p, pts) for p in polys], polys, mb.transcript(), lie)
            out.append(mb)
        cases = [("leaf", [small_vals(1 << n, j) for j in range(m_)]),
                 ("poly", [[5 + j] * (1 << n) for j in range(m_)])]
        if m_ == 1:
            cases.append(("last_elem", [[5] * (1 << n)]))
        for where, polys in cases:
            mb = Member("batched_pcs", (m_, n), ("noncanonical", where), None, {"K11"}, start)
            mb.proof = forge_batched_pcs(pts, [_mle(p, pts) for p in polys], polys, mb.transcript(), mb.lie)
            out.append(mb)
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """Every FRI / PCS / batched member, built once."""
    return tuple(_fri_members() + _pcs_members() + _batched_fri_members() + _batched_pcs_members())


SYSTEM_NAMES = ("pythagorean", "lin1")
SYSTEM_LIES = (None, "wrong_total_consistent", "other_trace")
PHASED_NAMES = ("lin1", "quad3", "pythagorean")  # lin1: P = W = 1; quad3: P < W; P = W without sums
PHASED_LIES = {"lin1": (None, "wrong_total_consistent", "wrong_column_sum_consistent", "other_trace_1"),
               "quad3": (None, "wrong_total_consistent", "wrong_column_sum_consistent", "other_trace_1",
                         "other_trace_2"),
               "pythagorean": (None, "wrong_total_consistent", "other_trace_1")}
