"""Operands that reach the butterflies' cold path (tools/gen_bfly.py: the
ripples the asm leaves out, flags E / FA / FD), found on the CPU with the
generator's integer model.  Shared by test_bfly_short_chain.py and
test_ntt_rare_paths_gpu.py; not a test module."""
import functools
import importlib.util
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def gen():
    spec = importlib.util.spec_from_file_location("gen_bfly", os.path.join(ROOT, "tools", "gen_bfly.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def omega4(inverse=False):
    """g^(n/4) of the forward transforms (oracle.field.pow_2_generator is
    3^((M-1)/n) for every n), or its inverse."""
    G = gen()
    w = pow(3, (G.M - 1) >> 2, G.M)
    return pow(w, G.M - 2, G.M) if inverse else w


@functools.lru_cache(maxsize=None)
def e_operands(w, count=4, seed=1):
    """Canonical v whose product w v loses the carry out of limb 2 of the
    fold (flag E): a search from a seeded start, about 2^17 steps per hit.
    A step adds 1 to limb 3 of v, so the unreduced product sum_k v_k B_k moves
    by B_3 and needs no recomputation; the model confirms every hit."""
    G = gen()
    rng = random.Random(seed)
    B = [w * (1 << (32 * k)) % G.M for k in range(4)]
    m96 = (1 << 96) - 1
    out = []
    while len(out) < count:
        v = rng.randrange(G.M >> 1)
        P = sum(vk * B[k] for k, vk in enumerate(G.limbs(v)))
        while v + (1 << 96) < G.M and len(out) < count:
            v += 1 << 96
            P += B[3]
            if ((P & m96) + (P >> 128) * G.C) >> 96:
                assert G.model(0, v, w)[2] == 1
                out.append(v)
    return tuple(out)


def fa_pair(a=0, b=0):
    """(u, v) whose sum wraps 2^128 and whose + C then carries out of limb 1
    (flag FA): u + v = 2^128 + 2^64 - 1 - (a - b), 0 <= b <= a < C."""
    G = gen()
    assert 0 <= b <= a < G.C
    return G.M - 1 - a, (1 << 64) + G.C + b


def fd_pair(a=0, b=0):
    """(u, v) whose difference borrows and whose - C then borrows out of limb
    1 (flag FD): u - v = -2^64 + 5 + a + b, 5 + a + b < C."""
    G = gen()
    assert a >= 0 and b >= 0 and 5 + a + b < G.C
    return a, (1 << 64) - 5 - b


# (v, w) whose full product (kind f) loses the borrow out of limb 1 of its
# second fold (flag G): found once by a seeded random search with
# full_product_g below, about 2^20 draws per hit; the tests confirm each pair
# with that model and with the emulated asm.
G_PAIRS_F = (
    (0xa000f7613b1f447d6f150c5591b17439, 0x28c73f5a4a485b32ca03e3b41de4435e),
    (0x5c91f04f7485ac314528407b76ae494a, 0xa870caa5821945e4f623f796dcd4613a),
    (0x55859b7dd49f021c25d26584d82b7236, 0x4b290dc9c78b02cbafdc6018693130d7),
    (0xa460053472275daf527a6a6e38f98030, 0xfda85a2a6abfce3095aad099cd3a950d),
)
# the same for the product by expanded multiples (kind p): w v = 2^128, so the
# low word is 0, T = 1 and both low limbs borrow
G_PAIR_P = (2, 1 << 127)


def full_product_g(v, w):
    """Flag G of the full product v w on integers: Z - H = L + H C with its
    top T = (tl, th); G is the borrow out of limb 1 of (Z - H) - T."""
    m32 = (1 << 32) - 1
    t = v * w
    x = (t & ((1 << 128) - 1)) + (t >> 128) * gen().C
    T = x >> 128
    return 1 if ((x >> 32) & m32) < (T >> 32) + (1 if (x & m32) < (T & m32) else 0) else 0
