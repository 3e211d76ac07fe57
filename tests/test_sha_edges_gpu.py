"""SHA-256 edges of the device code, bit for bit against hashlib.

The device transcript (transcript_dev.hpp: dsha2l_step<4> / <8>, dsha_update,
dsha_final; transcript_absorb_kernel, fri_last_kernel, sumcheck_round_kernel)
at every buffer fill: the word path from each of the 16 word positions, the
straddle of a block boundary, the second compression of the finalising clone
when the padded words leave no room for the length, the byte path of a length
or a source that is not a multiple of 4, and the high word of the bit length.
The provers that keep the transcript on the device, started from a transcript
that already holds a label of every alignment.  The generic Merkle leaves
(merkle.hip: leaf_bytes_kernel, leaf_batch_kernel) at the padding edges
55 / 56 / 63 / 64 / 119 / 120, items that straddle a block, trees large enough
for subtree_kernel, and mlh_merkle_open with many indices in one call.

References: hashlib.sha256, oracle/transcript.py, oracle/merkle.py,
oracle/field.py (and the oracle provers built on them).  Every comparison is
exact equality.
"""
import ctypes
import hashlib
import os
import random
import re
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import field as F  # noqa: E402  (checker only)
from oracle import fri as OF  # noqa: E402
from oracle import merkle as OM  # noqa: E402
from oracle import pcs as OP  # noqa: E402
from oracle import polynomials as OPL  # noqa: E402
from oracle import sumcheck as OS  # noqa: E402
from oracle import transcript as OT  # noqa: E402

from multilinear_amd import _lib  # noqa: E402
from multilinear_amd import device as D  # noqa: E402
from multilinear_amd import fri as MF  # noqa: E402
from multilinear_amd import merkle_tree as MM  # noqa: E402
from multilinear_amd import multilinear_pcs as MP  # noqa: E402
from multilinear_amd import sumcheck as MS  # noqa: E402
from multilinear_amd.transcript import DeviceTranscript, Transcript  # noqa: E402

M = F.M
_R = random.Random(0x5A17)
PRIOR = bytes(_R.randrange(256) for _ in range(192))  # bytes absorbed on the host first
DATA = bytes(_R.randrange(256) for _ in range(208))   # bytes absorbed on the device
TAIL7 = bytes(_R.randrange(256) for _ in range(7))    # absorbed on the host afterwards

# prior lengths: every fill of the first block and the first words of the
# second, and the fills 55 / 56 / 63 / 0 of later blocks
L0S = list(range(68)) + [119, 120, 127, 128, 191]
NS = [0, 1, 2, 3, 4, 5, 8, 12, 15, 16, 17, 20, 31, 32, 33, 48, 55, 56, 60, 63, 64, 65, 96, 127, 128,
      129, 200]


def dev(values):
    return D.to_device(D.ints_to_limbs(values))


def host(t):
    return D.limbs_to_ints(D.from_device(t))


def u8dev(b):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to("cuda:0")


def host_transcript(prior):
    t = Transcript()
    t.absorb(prior)
    return t


def oracle_transcript(prior):
    t = OT.Transcript()
    t.absorb(prior)
    return t


def assert_state(dt, absorbed, what):
    """The device state, copied back, is the SHA-256 state after `absorbed`:
    its digest pins h, buf and len together; 7 more bytes absorbed on the host
    show the buffer content (not only the padded clone) is right."""
    back = dt.to_host()
    assert back.random() == hashlib.sha256(absorbed).digest(), what
    back.absorb(TAIL7)
    assert back.random() == hashlib.sha256(absorbed + TAIL7).digest(), what


# ---- 1. device absorb from every fill --------------------------------------------

def _absorb_sweep(n, off):
    src_all = u8dev(DATA)
    assert src_all.data_ptr() % 4 == 0
    src = src_all[off:off + n] if n else src_all
    data = DATA[off:off + n]
    r = D.empty(1)
    dt = DeviceTranscript()
    for l0 in L0S:
        prior = PRIOR[:l0]
        want_r = oracle_transcript(prior + data).next_challenge()
        for with_r in (True, False):
            what = "L0=%d n=%d offset=%d challenge=%s" % (l0, n, off, with_r)
            dt.load(host_transcript(prior))
            r.fill_(-1)  # 2^128 - 1: no field element
            dt.absorb(src, r if with_r else None, nbytes=n)
            assert host(r) == [want_r if with_r else 2**128 - 1], what
            assert_state(dt, prior + data, what)


@pytest.mark.parametrize("n", NS)
def test_device_absorb_every_fill(n):
    """mlh_device_transcript_absorb of n device bytes into a state that holds
    L0 host bytes, for every L0: n = 16 / 32 from a fill that is a multiple of
    4 run dsha2l_step<4> / <8> (each word position, the straddle, the second
    compression when the padding starts at word 14 or 15), from any other fill
    its one-lane byte fallback; every other n runs dsha_update + dsha_final.
    With and without a challenge pointer."""
    _absorb_sweep(n, 0)


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("n", [16, 32])
def test_device_absorb_unaligned_source(n, off):
    """n = 16 / 32 from a source that is not 4-byte aligned: the kernel must
    take the byte path (a word load there would read other bytes)."""
    _absorb_sweep(n, off)


def test_device_absorb_zero_bytes_null_source():
    """n = 0 with a null source is valid: the state is unchanged and the
    challenge is next_challenge() of the prior bytes."""
    r = D.empty(1)
    dt = DeviceTranscript()
    for l0 in (0, 3, 56, 64):
        prior = PRIOR[:l0]
        dt.load(host_transcript(prior))
        r.fill_(-1)
        dt.absorb(None, r, nbytes=0)
        assert host(r) == [oracle_transcript(prior).next_challenge()], l0
        assert_state(dt, prior, "L0=%d" % l0)


@pytest.mark.parametrize("n", [16, 32])
def test_device_absorb_chain(n):
    """Five consecutive word-path absorbs on one device state, a challenge
    after each: from each aligned fill the chain walks the buffer positions,
    the straddles and the two-compression finalisations in sequence, every step
    starting from the state the step before wrote."""
    src_all = u8dev(DATA)
    r = D.empty(1)
    dt = DeviceTranscript()
    for l0 in [x for x in L0S if x % 4 == 0]:
        prior = PRIOR[:l0]
        dt.load(host_transcript(prior))
        ot = oracle_transcript(prior)
        absorbed = prior
        for i in range(5):
            chunk = DATA[n * i:n * (i + 1)]
            r.fill_(-1)
            dt.absorb(src_all[n * i:n * (i + 1)], r)
            ot.absorb(chunk)
            absorbed += chunk
            assert host(r) == [ot.next_challenge()], "L0=%d n=%d step %d" % (l0, n, i)
        assert_state(dt, absorbed, "L0=%d n=%d" % (l0, n))


# ---- 2. bit length above 2^32 ------------------------------------------------------

BIG = 1 << 29  # bytes: the bit length 2^32 sets the length field's high word


@pytest.fixture(scope="module")
def big_prefix():
    """(host transcript, hashlib state, seconds of the host absorb) after 2^29
    zero bytes; neither state is modified by the tests (they clone)."""
    chunk = bytes(1 << 22)
    t0 = time.perf_counter()
    tr = Transcript()
    for _ in range(BIG // len(chunk)):
        tr.absorb(chunk)
    secs = time.perf_counter() - t0
    h = hashlib.sha256()
    for _ in range(BIG // len(chunk)):
        h.update(chunk)
    return tr, h, secs


def test_bit_length_above_2_32(big_prefix):
    """The length field's high word (w[14]) in dsha2l_step (16- and 32-byte
    absorbs), dsha_final's byte path (5 bytes) and sha256_pad_kw (the
    padding-only blocks of mlh_sumcheck_prove_eq, whose second round ends on a
    block boundary) once more than 2^32 bits have been absorbed."""
    tr, h, secs = big_prefix
    print("host absorb of 2^29 bytes: %.2f s" % secs)
    assert tr.random() == h.digest()
    ot = OT.Transcript()
    ot.state = h.copy()
    src_all = u8dev(DATA)
    r = D.empty(1)
    dt = DeviceTranscript(tr)
    off = 0
    for n in (16, 32, 5):
        r.fill_(-1)
        dt.absorb(src_all[off:off + n], r)
        ot.absorb(DATA[off:off + n])
        assert host(r) == [ot.next_challenge()], n
        back = dt.to_host()
        assert back.random() == ot.random(), n
        off += n
    back.absorb(TAIL7)
    ot.absorb(TAIL7)
    assert back.random() == ot.random()
    # sumcheck from the 2^29-byte state: 3 rounds of 32 bytes
    n = 3
    rnd = random.Random(29)
    ev = [rnd.randrange(M) for _ in range(1 << n)]
    pts = [rnd.randrange(M) for _ in range(n)]
    total = OPL.mle_evaluate(ev, pts)
    ot = OT.Transcript()
    ot.state = h.copy()
    tables = OS.SumcheckTables.build_tables_for_pcs(pts, ev)
    prev, want_polys, want_rs = total, [], []
    for _ in range(n):
        nz, rr, prev = tables.compute_sumcheck_polynomial(prev, ot)
        want_polys.append(tuple(nz))
        want_rs.append(rr)
    t2 = tr.clone()
    polys, rs = MS.SumcheckTables.build_tables_for_pcs(pts, dev(ev)).compute_sumcheck_polynomials(total, t2)
    assert polys == want_polys and rs == want_rs
    assert t2.random() == ot.random()


# ---- 3. mlh_device_fri_last ----------------------------------------------------------

def test_device_fri_last_every_fill():
    """fri_last_kernel from every fill 0..67: flag = (a != b) (a difference in
    any one limb counts), last = a, and the state absorbed LE16(a) --
    dsha2l_step<4> without a challenge, or its byte fallback."""
    import torch

    rnd = random.Random(31)
    a1, a2 = rnd.randrange(1 << 120), rnd.randrange(M)
    pairs = [(0, 0), (0, 1), (M - 1, M - 1), (M - 1, 0), (0, M - 1), (M - 1, M - 2), (a1, a1), (a2, a2),
             (a1, a2), (a2, a1)] + [(a1, a1 ^ (1 << (32 * k + 7))) for k in range(4)]
    vals = dev([v for p in pairs for v in p])
    flag = torch.empty(1, dtype=torch.int32, device="cuda:0")
    last = D.empty(1)
    dt = DeviceTranscript()
    for l0 in range(68):
        prior = PRIOR[:l0]
        ht = host_transcript(prior)
        for i, (a, b) in enumerate(pairs):
            what = "L0=%d pair %d" % (l0, i)
            dt.load(ht)
            flag.fill_(0x5A5A5A5A)
            last.fill_(-1)
            dt.fri_last(vals[2 * i:2 * i + 2], flag, last)
            assert int(flag.cpu()[0]) == (1 if a != b else 0), what
            assert host(last) == [a], what
            assert_state(dt, prior + F.to_bytes(a), what)


# ---- 4. mlh_device_sumcheck_round ------------------------------------------------------

def _red_threads():
    src = os.path.join(os.path.dirname(os.path.abspath(MM.__file__)), "csrc", "sc_dev.hpp")
    with open(src) as f:
        return int(re.search(r"constexpr\s+int\s+kRedThreads\s*=\s*(\d+)\s*;", f.read()).group(1))


KRED = _red_threads()  # sumcheck_round_kernel's workgroup: its reduction strides by this
NPAIRS = sorted({1, 2, 3, 63, 64, 65, KRED - 1, KRED, KRED + 1, 1000})
SC_L0 = [0, 3, 4, 24, 28, 32, 36, 56, 60, 61]
INV2 = F.inv(2)


@pytest.mark.parametrize("npairs", NPAIRS)
def test_device_sumcheck_round(npairs):
    """Three rounds back to back on one device state and one device claim,
    against the closed form in Python integers: s1 = sum p[2i], s2 = sum
    p[2i+1], e0 = prev - s1, c2 = (s2 - 2 s1 + e0) / 2, c1 = s1 - e0 - c2,
    absorb LE16(c1) || LE16(c2), r = next_challenge(), prev' = e0 + r (c1 + c2 r).
    The fills put dsha2l_step<8> at a straddle (36, 56, 60), a two-compression
    finalisation (24, 28, 56, 60), a block-completing absorb (32) and the byte
    fallback (3, 61)."""
    rnd = random.Random(400 + npairs)
    rounds = []
    for _ in range(3):
        p = [rnd.randrange(M) for _ in range(2 * npairs)]
        p[0], p[-1] = 0, M - 1
        if npairs >= 3:
            p[2], p[3] = M - 1, M - 1
            p[-3] = 0
        rounds.append(p)
    pool = dev([v for p in rounds for v in p])
    claims = [0, M - 1] + [rnd.randrange(M) for _ in range(len(SC_L0) - 2)]
    poly, r = D.empty(2), D.empty(1)
    dt = DeviceTranscript()
    for l0, claim in zip(SC_L0, claims):
        prior = PRIOR[:l0]
        dt.load(host_transcript(prior))
        ot = oracle_transcript(prior)
        absorbed = prior
        prev = dev([claim])
        for k, p in enumerate(rounds):
            what = "npairs=%d L0=%d round %d" % (npairs, l0, k)
            poly.fill_(-1)
            r.fill_(-1)
            dt.sumcheck_round(pool[2 * npairs * k:2 * npairs * (k + 1)], npairs, prev, poly, r)
            s1, s2 = sum(p[0::2]) % M, sum(p[1::2]) % M
            e0 = (claim - s1) % M
            c2 = (s2 - 2 * s1 + e0) * INV2 % M
            c1 = (s1 - e0 - c2) % M
            msg = F.to_bytes(c1) + F.to_bytes(c2)
            ot.absorb(msg)
            absorbed += msg
            rr = ot.next_challenge()
            claim = (e0 + rr * (c1 + c2 * rr)) % M
            assert host(poly) == [c1, c2], what
            assert host(r) == [rr], what
            assert host(prev) == [claim], what
            assert_state(dt, absorbed, what)


# ---- 5. whole provers from a non-empty transcript ------------------------------------------

LABEL_LENS = list(range(0, 61, 4)) + [1, 2, 3, 61, 62, 63]


def rand_vals(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(M) for _ in range(n)]


class fused_max:
    """mlh_set_pcs_fused_max for the block: 0 sends the PCS through the
    one-round-per-launch (cooperative) path, 24 is the default."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        ctx = D.context()
        D.check(D.lib().mlh_set_pcs_fused_max(ctx, self.v), ctx)

    def __exit__(self, *exc):
        ctx = D.context()
        D.check(D.lib().mlh_set_pcs_fused_max(ctx, 24), ctx)
        return False


def _assert_queries(got_fri, want_fri):
    for q in range(_lib.NUM_QUERIES):
        gq, wq = got_fri.query(q), want_fri.queries[q]
        assert len(gq) == len(wq)
        for (gv, gs), (wv, wpath) in zip(gq, wq):
            assert gv == wv
            assert gs == [s for s, _ in wpath]


def _oracle_fri_proof(got):
    """The device proof's own records as an oracle FriProof (the directions of
    a path are the bits of the index it opens)."""
    queries = []
    for q, idx in enumerate(got.query_indices):
        cur, cur_n, paths = idx, 1 << (got.log_code - 1), []
        for val, sibs in got.query(q):
            paths.append((val, [(s, OM.LEFT if (cur >> i) & 1 else OM.RIGHT) for i, s in enumerate(sibs)]))
            cur_n //= 2
            cur %= cur_n
        queries.append(paths)
    return OF.FriProof(got.commitments, queries, got.last_elem, got.last_random)


def _oracle_fri_verify(proof, label):
    """FriProof::verify (fri/mod.rs:287-309) by the oracle, on a transcript
    that starts with `label`."""
    tr = oracle_transcript(label)
    rs = []
    for root in proof.commitments:
        tr.absorb(root)
        rs.append(tr.next_challenge())
    tr.absorb(F.to_bytes(proof.last_elem))
    return proof.verify_queries(tr, rs)


@pytest.fixture(scope="module")
def fri_case():
    log_n = 5
    gp = F.pow_2_generator_powers(log_n + 1)
    return gp, OF.reed_solomon(rand_vals(1 << log_n, 501), gp[1])


@pytest.mark.parametrize("label_len", LABEL_LENS)
def test_fri_prove_from_labelled_transcript(fri_case, label_len):
    """FriProof.prove at log_n = 5 (the device commit loop: root absorbs,
    challenges, the last element) from a transcript that holds a label."""
    gp, code = fri_case
    label = PRIOR[:label_len]
    otr = oracle_transcript(label)
    want = OF.FriProof.prove(code, gp, otr)
    tr = host_transcript(label)
    got = MF.FriProof.prove(dev(code), tr)
    assert got.commitments == want.commitments
    assert got.last_elem == want.last_elem
    assert got.last_random == want.last_random
    _assert_queries(got, want)
    assert tr.next_challenge() == otr.next_challenge()
    assert _oracle_fri_verify(_oracle_fri_proof(got), label)
    assert _oracle_fri_verify(want, label)
    assert got.verify() == (label_len == 0)  # verify() starts from an empty transcript


def _oracle_sumcheck(ev, pts, total, label):
    tables = OS.SumcheckTables.build_tables_for_pcs(pts, ev)
    otr = oracle_transcript(label)
    prev, polys, rs = total, [], []
    for _ in range(len(pts)):
        nz, r2, prev = tables.compute_sumcheck_polynomial(prev, otr)
        polys.append(tuple(nz))
        rs.append(r2)
    return polys, rs, otr


_sumcheck_cases = {}


def _sumcheck_case(n):
    """(evaluations, points, claimed sum, device evaluations, device eq table), built once."""
    if n not in _sumcheck_cases:
        ev, pts = rand_vals(1 << n, 510 + n), rand_vals(n, 520 + n)
        _sumcheck_cases[n] = (ev, pts, OPL.mle_evaluate(ev, pts), dev(ev), dev(OS.eq_table(pts)))
    return _sumcheck_cases[n]


@pytest.mark.parametrize("label_len", LABEL_LENS)
@pytest.mark.parametrize("n", [3, 13])
def test_sumcheck_prove_from_labelled_transcript(n, label_len):
    """mlh_sumcheck_prove on materialised tables: n = 3 is the LDS tail launch
    alone, n = 13 one sumcheck_round_kernel launch (its partial sums from HBM)
    and then the tail."""
    ev, pts, total, dev_ev, dev_eq = _sumcheck_case(n)
    label = PRIOR[:label_len]
    want_polys, want_rs, otr = _oracle_sumcheck(ev, pts, total, label)
    mt = MS.SumcheckTables(dev_ev.clone(), dev_eq.clone())  # both given: folded in place
    tr = host_transcript(label)
    polys, rs = mt.compute_sumcheck_polynomials(total, tr)
    assert polys == want_polys and rs == want_rs
    assert tr.random() == otr.random()
    assert tr.next_challenge() == otr.next_challenge()


@pytest.mark.parametrize("label_len", LABEL_LENS)
def test_sumcheck_prove_eq_from_labelled_transcript(label_len):
    """mlh_sumcheck_prove_eq at n = 14: the cooperative one-workgroup kernels
    (a two-round head group, the 12-round eq tail) with their transcript wave."""
    n = 14
    ev, pts, total, dev_ev, _ = _sumcheck_case(n)
    label = PRIOR[:label_len]
    want_polys, want_rs, otr = _oracle_sumcheck(ev, pts, total, label)
    mt = MS.SumcheckTables.build_tables_for_pcs(pts, dev_ev)  # (the evaluations are only read)
    tr = host_transcript(label)
    polys, rs = mt.compute_sumcheck_polynomials(total, tr)
    assert polys == want_polys and rs == want_rs
    assert tr.random() == otr.random()
    assert tr.next_challenge() == otr.next_challenge()


_pcs_oracle = {}


def _pcs_case(label_len):
    """The oracle's PCS proof at n = 8 from the label, its transcript's next
    challenge afterwards (shared by the two device paths)."""
    n = 8
    if "case" not in _pcs_oracle:
        ev, pts = rand_vals(1 << n, 530), rand_vals(n, 531)
        _pcs_oracle["case"] = (ev, pts, OPL.mle_evaluate(ev, pts))
    ev, pts, out = _pcs_oracle["case"]
    if label_len not in _pcs_oracle:
        otr = oracle_transcript(PRIOR[:label_len])
        want = OP.PCSProof.prove(pts, out, ev, otr)
        _pcs_oracle[label_len] = (want, otr.next_challenge())
    return (ev, pts, out) + _pcs_oracle[label_len]


@pytest.mark.parametrize("label_len", LABEL_LENS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_round"])
def test_pcs_prove_from_labelled_transcript(fused, label_len):
    """mlh_pcs_prove at n = 8 with the rounds off the transcript chain (the
    launch that writes a root absorbs root and round polynomial) and on the
    one-round-per-launch path (sumcheck_round_kernel, then the root absorb)."""
    ev, pts, out, want, want_next = _pcs_case(label_len)
    label = PRIOR[:label_len]
    tr = host_transcript(label)
    with fused_max(24 if fused else 0):
        got = MP.PCSProof.prove(pts, out, dev(ev), tr)
    assert got.sumcheck_polynomials == [tuple(p) for p in want.sumcheck_polynomials]
    assert got.fri_proof.commitments == want.fri_proof.commitments
    assert got.fri_proof.last_elem == want.fri_proof.last_elem
    assert got.fri_proof.last_random == want.fri_proof.last_random
    _assert_queries(got.fri_proof, want.fri_proof)
    assert tr.next_challenge() == want_next
    assert got.verify(host_transcript(label))
    assert want.verify(oracle_transcript(label))
    if label_len:
        assert not got.verify(Transcript())


# ---- 6. generic Merkle leaves ----------------------------------------------------------------

ITEM_LENS = [1, 31, 32, 55, 56, 57, 63, 64, 65, 119, 120, 128, 200]
COUNTS = [1, 2, 64, 128, 256, 2048, 4096]  # 2048: the first generic tree that runs subtree_kernel
BATCHES = [(1, 1), (2, 32), (4, 16), (16, 32), (5, 11), (7, 8), (4, 14), (3, 21), (9, 7), (3, 40),
           (2, 100)]  # message lengths 1, 64, 64, 512, 55, 56, 56, 63, 63, 120, 200
BATCH_COUNTS = [1, 8, 256, 2048]


def _items(fill, count, ln):
    """count items of ln bytes: seeded random bytes (fill = a seed), or all
    one byte value (fill = bytes of length 1)."""
    if isinstance(fill, bytes):
        return [fill * ln] * count
    raw = np.random.default_rng(fill).integers(0, 256, size=count * ln, dtype=np.uint8).tobytes()
    return [raw[i * ln:(i + 1) * ln] for i in range(count)]


def _assert_tree(got, want, what):
    """Every layer of the device tree against the oracle's, and the root."""
    gl = got.layers()
    assert len(gl) == len(want.layers), what
    for lvl, (a, b) in enumerate(zip(gl, want.layers)):
        assert a.shape == (len(b), 32), what
        if a.tobytes() != b"".join(b):
            bad = [i for i in range(len(b)) if bytes(a[i]) != b[i]]
            assert False, "%s: layer %d differs at %d nodes, first %d" % (what, lvl, len(bad), bad[0])
    assert got.root() == want.root(), what


@pytest.mark.parametrize("item_len", ITEM_LENS)
def test_merkle_commit_item_lengths(item_len):
    """Merkle.commit over items of item_len bytes (leaf_bytes_kernel): one
    block up to 55 bytes, two from 56 (at 63 the 0x80 is the first block's last
    byte, at 64 it opens the second), three from 120; every layer of every tree
    size, the two-leaf and one-leaf trees included."""
    for count in COUNTS:
        data = _items(1000 * item_len + count, count, item_len)
        got, want = MM.Merkle.commit(data), OM.Merkle.commit(data)
        _assert_tree(got, want, "item_len=%d count=%d" % (item_len, count))
        if count == 1:
            leaf = hashlib.sha256(data[0]).digest()
            assert [bytes(x) for layer in got.layers() for x in layer] == [leaf]
            assert got.root() == leaf
    for fill in (b"\xff", b"\x00"):
        for count in (1, 64):
            data = _items(fill, count, item_len)
            _assert_tree(MM.Merkle.commit(data), OM.Merkle.commit(data),
                         "item_len=%d count=%d fill=%r" % (item_len, count, fill))


@pytest.mark.parametrize("m,item_len", BATCHES)
def test_merkle_batch_commit_item_lengths(m, item_len):
    """Merkle.batch_commit (leaf_batch_kernel): leaf i = SHA-256 of the m
    items data[j][i] concatenated -- the gather across batches, items that
    straddle a block boundary, concatenations on the padding edges; every
    layer, and batch_open's values and paths."""
    for count in BATCH_COUNTS:
        what = "m=%d item_len=%d count=%d" % (m, item_len, count)
        data = [_items(100000 * m + 1000 * item_len + 10 * count + j, count, item_len) for j in range(m)]
        got, want = MM.Merkle.batch_commit(data), OM.Merkle.batch_commit(data)
        _assert_tree(got, want, what)
        for i in sorted({0, 1, count // 2, count - 1} & set(range(count))):
            value, path = got.batch_open(i)
            assert (value, path) == OM.batch_open(want, i), "%s index %d" % (what, i)
            assert OM.batch_verify(value, path, want.root(), i), "%s index %d" % (what, i)
    for fill in (b"\xff", b"\x00"):
        data = [_items(fill, 8, item_len) for _ in range(m)]
        _assert_tree(MM.Merkle.batch_commit(data), OM.Merkle.batch_commit(data),
                     "m=%d item_len=%d fill=%r" % (m, item_len, fill))


# ---- 7. mlh_merkle_open with many indices --------------------------------------------------------

SENTINEL = 0xA5


def _open_many(tree, leaves, idx, pad=64):
    """mlh_merkle_open once for all of idx -> (status, the out buffer: len(idx)
    records and `pad` sentinel bytes behind them)."""
    depth = leaves.bit_length() - 1
    size = 32 * depth * len(idx) + pad
    out = (ctypes.c_uint8 * size).from_buffer_copy(bytes([SENTINEL]) * size)
    arr = (ctypes.c_uint64 * len(idx))(*idx)
    ctx = D.context()
    st = D.lib().mlh_merkle_open(ctx, D.ptr(tree.layers_flat), leaves, arr, len(idx), out)
    return st, bytes(out)


def _index_lists(leaves, seed):
    mid = leaves // 2
    rnd = random.Random(seed)
    lists = [[0], [leaves - 1], [0, leaves - 1], [leaves - 1, leaves - 1], [mid, mid ^ 1]]
    for nq in (65, 300):
        idx = [0, leaves - 1, 0, leaves - 1, mid, mid ^ 1, mid, 1, 0]
        while len(idx) < nq:
            i = rnd.randrange(leaves)
            idx += [i, i ^ 1, i]  # a sibling pair and a repeat
        lists.append(idx[:nq])
    return lists


@pytest.mark.parametrize("leaves", [2, 8, 4096])
def test_merkle_open_many_indices(leaves):
    """merkle_path_kernel runs one workgroup per query: nq = 1, 2, 65 and 300
    records from one call, each the oracle's path for its index, and nothing
    written behind the last record."""
    data = _items(7000 + leaves, leaves, 8)
    tree, want = MM.Merkle.commit(data), OM.Merkle.commit(data)
    assert tree.root() == want.root()
    rec = 32 * (leaves.bit_length() - 1)
    for idx in _index_lists(leaves, leaves):
        st, raw = _open_many(tree, leaves, idx)
        assert st == _lib.MLH_OK
        for q, i in enumerate(idx):
            assert raw[q * rec:(q + 1) * rec] == b"".join(s for s, _ in want.open(i)[1]), \
                "leaves=%d nq=%d record %d (index %d)" % (leaves, len(idx), q, i)
        assert raw[len(idx) * rec:] == bytes([SENTINEL]) * 64


def test_merkle_open_one_leaf_tree():
    """A one-leaf tree has empty paths: MLH_OK and the out buffer untouched."""
    tree = MM.Merkle.commit([b"one leaf"])
    st, raw = _open_many(tree, 1, [0, 0, 0], pad=96)
    assert st == _lib.MLH_OK
    assert raw == bytes([SENTINEL]) * 96
