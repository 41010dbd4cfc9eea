"""Designed inputs for the device carry scan (prmers_amd/csrc/canon.hip) -- TEST INFRASTRUCTURE ONLY.

After its local passes the scan sees a 0/1 carry chain: a digit generates a carry iff it equals 2^w and passes one on iff it equals
2^w - 1.  Random digits do either with probability ~2^-w, so the block aggregates (k_scan_blocks), the carry into every block
(k_scan_top: 256 threads, each over a stretch of `per` = ceil(nblocks / 256) blocks) and k_apply only see carries in vectors made
for them.  This module makes such vectors and their canonical forms BY CONSTRUCTION, without carrying anything:

    sum_{j = a .. a+L-1} (2^w_j - 1) 2^off_j  +  2^off_a  =  2^off_(a+L)        (indices cyclic, 2^p = 1)

so a chain (a, L) -- L digits of all ones from digit a on, plus one unit on digit a -- is worth exactly one unit on the digit e behind
it: the canonical form has zeros on the chain and digit e one higher (its bit 0 is cleared beforehand, so nothing moves further).
tests/test_canon_cases.py checks the pairs against a sequential carry on Python integers at small geometries of the same shape.
"""
import collections

import numpy as np

BLOCK = 4096      # digits per block of the scan (canon.hip kBlockDigits)
TOP_THREADS = 256  # threads of k_scan_top, one stretch of blocks each
MIN_STRETCHES = 53  # the chain table below names stretches up to 52

# d: input digits (each <= 2^w).  t: the canonical digits as the engines hand them out -- for the value 2^p - 1 that is all ones
# (zero = True: the value is 0, registers compare equal to 0).  touched: where d and t differ.
Case = collections.namedtuple("Case", "name d t touched zero")


def widths(p, n):
    """w[j] = ceil(p (j + 1) / n) - ceil(p j / n)"""
    j = np.arange(n + 1, dtype=np.uint64)
    c = (j * np.uint64(p) + np.uint64(n - 1)) // np.uint64(n)
    return (c[1:] - c[:-1]).astype(np.uint64)


def geometry(n, B=BLOCK):
    """(blocks, blocks per stretch, digits per stretch, stretches in use)"""
    nb = -(-n // B)
    per = -(-nb // TOP_THREADS)
    S = per * B
    return nb, per, S, -(-n // S)


def stretch_start(n, B, k):
    """first digit of stretch k; sizes with fewer stretches than the table names get the stretch indices scaled down"""
    nb, per, S, ns = geometry(n, B)
    return (k if ns >= MIN_STRETCHES else k * ns // MIN_STRETCHES) * S


def chain_table(n, B=BLOCK):
    """name -> [(first digit, length)]: where the chains start and end relative to thread, block and stretch edges"""
    nb, per, S, ns = geometry(n, B)

    def s(k):
        return stretch_start(n, B, k)

    return collections.OrderedDict([
        ("thread_block_stretch_edges", [(47, 2), (5 * B - 1, 2), (s(7) - 1, 2), (s(9) - 3, 3), (s(11), 1), (s(12) + B - 1, 1)]),
        ("inside_one_stretch_across_its_blocks", [(s(2) + 5, S - 10), (s(20) + B - 7, B + 14)]),
        ("exactly_one_stretch", [(s(4), S), (s(30), S - 1), (s(40) + 1, S - 1)]),
        ("several_stretches", [(s(3) + B // 2, 5 * S + 3), (s(50) - 1, 2 * S + 2)]),
        ("wrap_short", [(n - 2, 5)]),
        ("wrap_from_last_stretch", [(n - S - 3, 3 * S + 4)]),
        ("wrap_lands_on_digit0", [(n - B, B)]),
        ("almost_all", [(s(6) + 1, n - 1)]),
        ("full_loop_mid", [(s(6) + 1, n)]),
        ("full_loop_0", [(0, n)]),
        ("full_loop_last", [(n - 1, n)]),
    ])


def ones_of(w):
    return (np.uint64(1) << w) - np.uint64(1)


def base_digits(w, seed):
    """canonical, seeded random digits"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 62, w.size, dtype=np.uint64) & ones_of(w)


def from_chains(name, w, chains, seed):
    """The case of a list of disjoint chains (end digits included) over seeded random canonical digits."""
    n = w.size
    ones = ones_of(w)
    one = np.uint64(1)
    if len(chains) == 1 and chains[0][1] == n:   # the carry runs through every digit and comes back to where it started
        a = chains[0][0]
        d = ones.copy(); d[a] += one
        t = np.zeros(n, dtype=np.uint64); t[a] = one
        return Case(name, d, t, np.ones(n, dtype=bool), False)
    d = base_digits(w, seed)
    t = d.copy()
    touched = np.zeros(n, dtype=bool)
    for a, L in chains:
        if not 0 < L < n or not 0 <= a < n:
            raise ValueError("%s: chain (%d, %d) does not fit n = %d" % (name, a, L, n))
        idx = (a + np.arange(L + 1, dtype=np.int64)) % n   # the chain and the digit behind it
        if touched[idx].any():
            raise ValueError("%s: chain (%d, %d) overlaps another one" % (name, a, L))
        touched[idx] = True
        body, e = idx[:-1], idx[-1]
        d[body] = ones[body]
        d[a] += one
        d[e] &= ~one
        t[body] = 0
        t[e] = d[e] + one
    return Case(name, d, t, touched, False)


def iter_cases(n, w, B=BLOCK, seed=1):
    """Every designed vector for n digits of widths w, blocks of B digits, one at a time (a vector of a large size is tens of megabytes)."""
    w = np.asarray(w, dtype=np.uint64)
    assert w.size == n
    nb, per, S, ns = geometry(n, B)
    ones = ones_of(w)
    one = np.uint64(1)
    none = np.zeros(n, dtype=bool)
    table = chain_table(n, B)
    for k, (name, chains) in enumerate(table.items()):
        yield from_chains(name, w, chains, seed + k)
    # 2^p - 1 = 0: nothing generates and everything propagates; the engines' digit reads keep the all-ones vector
    yield Case("all_ones", ones.copy(), ones.copy(), none, True)
    # all ones but one digit: canonical already, and not zero
    for name, k in (("ones_hole_mid", stretch_start(n, B, 5) + B), ("ones_hole_0", 0), ("ones_hole_last", n - 1)):
        d = ones.copy(); d[k] -= one
        yield Case(name, d, d.copy(), none, False)
    # a long run of all ones that no carry enters (the digit before it is 0) next to a chain that does carry: the run must stay
    c = from_chains("propagate_without_generate", w, [(stretch_start(n, B, 8) + 3, S + 9)], seed + 100)
    lo, hi = stretch_start(n, B, 15) - 2, stretch_start(n, B, 17) + 2
    if c.touched[lo - 1:hi].any():
        raise ValueError("propagate_without_generate: the run overlaps the chain")
    for v in (c.d, c.t):
        v[lo:hi] = ones[lo:hi]
        v[lo - 1] = 0
    yield c


def cases(n, w, B=BLOCK, seed=1):
    return list(iter_cases(n, w, B, seed))


def merged(name, w, names, B=BLOCK, seed=1):
    """One vector with the chains of several table rows (they must be disjoint)."""
    w = np.asarray(w, dtype=np.uint64)
    table = chain_table(w.size, B)
    return from_chains(name, w, [ch for nm in names for ch in table[nm]], seed)


def low64(t, w):
    """the low 64 bits of the value of canonical digits t, on Python integers"""
    v, sh = 0, 0
    for tj, wj in zip(t[:64].tolist(), w[:64].tolist()):
        v |= int(tj) << sh
        sh += int(wj)
        if sh >= 64:
            break
    return v & ((1 << 64) - 1)


def local_passes(d, w, passes=3):
    """What the scan is handed: `passes` times d'[j] = (d[j] mod 2^w_j) + (d[j-1] >> w_(j-1)), cyclic (canon.hip k_local).  A digit above
    2^w after them raises the sticky "too wide" flag and sends the caller to the host carry; digits of at most 2^w cannot grow."""
    d = np.asarray(d, dtype=np.uint64)
    for _ in range(passes):
        d = (d & ones_of(w)) + np.roll(d >> w, 1)
    return d
