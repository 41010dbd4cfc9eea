"""The host digit arithmetic both engines share (prmers_amd/csrc/host_digits.hpp: strong carry with wrap-around, residue words <-> digits,
the fold of 2^p = 1, the all-ones test, res64) through tests/host/host_digits_query.cpp, judged by Python integers.  No GPU.

The checker is written independently: with V = sum d_j 2^offset_j, the canonical digits are zeros if V = 0, else the digits of
r = V mod 2^p - 1 if r != 0, else all ones; the words are r (0 for all ones).  All ones is therefore the one canonical vector that does not
survive pack_words / unpack_words: it packs to 0 by definition, and the round trip is checked against the digits of the words' value."""
import os
import random
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prmers_amd", "csrc")

# (p, n, widths): the smallest shapes that reach every branch -- 19/20 bits put pieces of three digits into one word, 38/39 bits have a
# digit that starts at bit >= 26 of a word and spans three words
SHAPES = [(127, 8, (15, 16)), (9941, 512, (19, 20)), (1279, 36, (35, 36)), (9941, 256, (38, 39))]


@pytest.fixture(scope="module")
def query():
    td = tempfile.mkdtemp(prefix="host_digits_")
    exe = os.path.join(td, "host_digits_query")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "host", "host_digits_query.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        return [(ln.split()[0], [int(x) for x in ln.split()[1:]]) for ln in out]
    return run


class Shape:
    def __init__(self, p, n):
        self.p, self.n, self.mp = p, n, (1 << p) - 1
        self.off = [-((-p * j) // n) for j in range(n + 1)]          # ceil(p j / n)
        self.w = [self.off[j + 1] - self.off[j] for j in range(n)]
        self.wc = (p + 31) // 32

    def value(self, d):
        return sum(x << o for x, o in zip(d, self.off))

    def digits(self, v):
        return [(v >> self.off[j]) & ((1 << self.w[j]) - 1) for j in range(self.n)]

    def ones(self):
        return [(1 << w) - 1 for w in self.w]

    def words(self, v):
        return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(self.wc)]


def carry_inputs(s, wide):
    ones = s.ones()
    cases = [s.digits(0), s.digits(1), s.digits(s.mp - 1), ones,
             [ones[0] + 1] + ones[1:],                                # carries through every digit, out of the last one and back in
             [1 << w for w in s.w]]
    rng = random.Random(s.p * 1000 + s.n)
    if wide:                                                          # over-wide digits: values just below 2^62
        cases.append([(1 << 62) - 1 - rng.randrange(1 << 20) for _ in s.w])
        cases.append([(1 << 62) - 1] * s.n)
    else:                                                             # w + 20 bits
        cases.append([rng.randrange(1 << (w + 20)) for w in s.w])
        cases.append([(1 << (w + 20)) - 1 for w in s.w])
    for k in range(32):                                               # half of them canonical, half with a few bits too many
        cases.append([rng.randrange(1 << (w + (3 if k & 1 else 0))) for w in s.w])
    return cases


@pytest.mark.parametrize("p,n,widths", SHAPES)
def test_carry_pack_unpack_res64_against_integers(query, p, n, widths):
    s = Shape(p, n)
    assert set(s.w) == set(widths) and sum(s.w) == p
    if widths == (19, 20):
        assert any(sum(1 for j in range(n) if s.off[j] < 32 * i + 32 and s.off[j + 1] > 32 * i) >= 3 for i in range(s.wc))
    if widths == (38, 39):
        assert any(s.off[j] % 32 >= 26 and s.off[j] % 32 + s.w[j] > 64 for j in range(n))
    cases = carry_inputs(s, wide=widths[0] > 32)
    out = query(["carry %d %d %s" % (p, n, " ".join(map(str, d))) for d in cases])
    assert len(out) == 5 * len(cases)
    for k, d in enumerate(cases):
        got = dict(out[5 * k:5 * k + 5])
        assert list(got) == ["carry", "ones", "res64", "words", "unpack"]
        v = s.value(d)
        r = v % s.mp
        want = s.digits(0) if v == 0 else s.digits(r) if r else s.ones()
        assert got["carry"] == want, (p, n, k)
        assert got["ones"] == [1 if want == s.ones() else 0], (p, n, k)
        assert got["res64"] == [s.value(want) & ((1 << 64) - 1)], (p, n, k)
        assert got["words"] == s.words(r), (p, n, k)
        assert got["unpack"] == s.digits(r), (p, n, k)
        if want != s.ones():
            assert got["unpack"] == want, (p, n, k)      # unpack_words(pack_words(x)) == x


@pytest.mark.parametrize("p,n,widths", SHAPES)
def test_fold_words_mod_mp(query, p, n, widths):
    s = Shape(p, n)
    rng = random.Random(p)
    values = [1 << p, (1 << p) + 5, (1 << (32 * s.wc)) - 1, 0, 5, s.mp, s.mp + 1] + [rng.randrange(1 << (32 * s.wc)) for _ in range(8)]
    out = query(["fold %d %s" % (p, " ".join(map(str, s.words(v)))) for v in values])
    for v, (tag, got) in zip(values, out):
        want = v
        while want >> p:                                  # 2^p = 1; 2^p - 1 itself stays (the digits' canonical form decides that one)
            want = (want & s.mp) + (want >> p)
        assert tag == "fold" and got == s.words(want), (p, hex(v))
        assert want % s.mp == v % s.mp
