"""Host side of the crafted-image tests (no GPU): the word helpers of tests/image_words.py against Python integers, the kernels and the
capacity of every case the GPU file uses, and the word classes its mode-3 generator really produces."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import image_words as iw
from image_words import CASES, EDGE_WORDS, P
from mul_sum_cases import ROW_KERNELS, sum_product_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prmers_amd", "csrc")
U64 = np.uint64


@pytest.fixture(scope="module")
def host_tool():          # (built the way tests/test_mul_sum_bounds.py builds its tools)
    td = tempfile.mkdtemp()

    def run(src, *args):
        exe = os.path.join(td, os.path.splitext(src)[0])
        if not os.path.exists(exe):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", src)])
        return subprocess.check_output([exe, *map(str, args)]).decode().splitlines()
    return run


@pytest.fixture(scope="module")
def shapes(host_tool):
    """{case: (n, q, c, sum_fast)} from plan.hpp"""
    lines = host_tool("sum_query.cpp", *["%d:%s" % (p, s) if s else p for p, s in CASES])
    out = {}
    for case, line in zip(CASES, lines):
        f = {k: int(v) for k, v in (t.split("=") for t in line.split())}
        assert f["p"] == case[0] and f["q"] == f["p"] // f["n"]
        out[case] = (f["n"], f["q"], f["c"], f["sum_fast"])
    return out


def words_under_test():
    rng = np.random.default_rng(20260)
    return [int(v) for v in EDGE_WORDS] + [int(v) for v in rng.integers(0, 2**64, size=10**4, dtype=U64)]


def test_edge_words_are_the_twelve_of_the_issue():
    assert EDGE_WORDS == [0, 1, 2**32 - 2, 2**32 - 1, 2**32, 2**63, P - 1, P, P + 1, 2**64 - 2**32, 2**64 - 2, 2**64 - 1]
    assert EDGE_WORDS[9] == P - 1 == EDGE_WORDS[6] and all(0 <= w < 2**64 for w in EDGE_WORDS)
    assert P == 0xFFFFFFFF00000001


def test_fold_against_integers():
    ws = words_under_test()
    got = iw.fold(np.array(ws, dtype=U64))
    assert got.dtype == U64 and [int(v) for v in got] == [w % P for w in ws]


def test_split_and_join_are_inverse_and_little_endian():
    rng = np.random.default_rng(1)
    buf = rng.integers(0, 256, size=8 * 16 + 8, dtype=np.uint8)
    words, tag = iw.split(buf)
    assert words.dtype == U64 and words.size == 16 and tag == buf[-8:].tobytes()
    assert int(words[3]) == int.from_bytes(buf[24:32].tobytes(), "little")
    back = iw.join(words, tag)
    assert back.dtype == np.uint8 and np.array_equal(back, buf)
    words[0] = U64(2**64 - 1)
    assert iw.join(words, tag)[:8].tolist() == [255] * 8 and np.array_equal(iw.join(words, tag)[8:], buf[8:])


def test_lift_against_integers_and_never_wraps():
    ws = words_under_test()
    for mask_of in (lambda i: True, lambda i: False, lambda i: i % 3 == 0):
        words = np.array(ws, dtype=U64)
        mask = np.array([bool(mask_of(i)) for i in range(len(ws))])
        count = iw.lift(words, mask)
        want, lifted = [], 0
        for w, m in zip(ws, mask):
            if m and w % P < 2**32 - 1:
                want.append(w % P + P)
                lifted += 1
            else:
                want.append(w)
        assert all(v < 2**64 for v in want)                          # the lifted word exists in 64 bits
        assert [int(v) for v in words] == want and count == lifted
        assert [int(v) % P for v in words] == [w % P for w in ws]    # the same field element everywhere
    # the two ends of the liftable range, and the first word that has no second representative
    words = np.array([0, 2**32 - 2, 2**32 - 1, P - 1], dtype=U64)
    assert iw.lift(words, np.ones(4, dtype=bool)) == 2
    assert [int(v) for v in words] == [P, 2**64 - 1, 2**32 - 1, P - 1]


def test_complement_against_integers_on_edge_pairs_and_random_words():
    ws = words_under_test()
    for A in (0, 1, 2**15 - 1, 2**32 - 2, 2**32 - 1):
        for plane in (True, False):
            R = np.array(ws, dtype=U64)
            mask = np.full(R.size, plane)
            S = iw.complement(A, R, mask)
            t = A if plane else 0
            for r, s in zip(ws, (int(v) for v in S)):
                assert 0 <= s < P and (r % P + s) % P == t, (A, plane, r, s)
    # every edge word against every edge word as (target, word): the complement of R to the canonical value of another edge word below 2^32
    for A in [w % P for w in EDGE_WORDS if w % P < 2**32]:
        S = iw.complement(A, np.array(EDGE_WORDS, dtype=U64), np.ones(len(EDGE_WORDS), dtype=bool))
        assert [(r % P + int(s)) % P for r, s in zip(EDGE_WORDS, S)] == [A] * len(EDGE_WORDS)


def test_lazy_sum_model_on_edge_pairs():
    """image_words.lazy_sum restates gf::add_lazy_any: a 64-bit word congruent to a + b for every pair of edge words"""
    a = [x for x in EDGE_WORDS for _ in EDGE_WORDS]
    b = [y for _ in EDGE_WORDS for y in EDGE_WORDS]
    for x, y, s in zip(a, b, iw.lazy_sum(np.array(a, dtype=U64), np.array(b, dtype=U64))):
        assert 0 <= s < 2**64 and s % P == (x + y) % P, (x, y, s)


def test_plane_a_accepts_both_representatives_and_refuses_anything_else():
    w = np.array([1, 0, P + 1, P, 1, P, P + 1, 0], dtype=U64)
    assert iw.plane_a(w).tolist() == [True, False, True, False, True, False, True, False]
    for bad in ([1, 0, 2, 0], [1, 1, 1, 0], [0, 0, 0, 1], [P - 1, 0, 1, 0]):
        with pytest.raises(AssertionError):
            iw.plane_a(np.array(bad, dtype=U64))


def test_constant_image_takes_scalars_and_arrays():
    mask = np.array([True, False, False, True])
    assert iw.constant_image(mask, 2**64 - 1, P).tolist() == [2**64 - 1, P, P, 2**64 - 1]
    ra = np.array([1, 2, 3, 4], dtype=U64)
    assert iw.constant_image(mask, ra, 0).tolist() == [1, 0, 0, 4]


def test_every_case_reaches_the_row_kernel_it_names(host_tool):
    lines = host_tool("plan_query.cpp", *["k:%d%s" % (p, ":" + s if s else "") for p, s in CASES])
    assert len(lines) == len(CASES) == len(iw.ROWS_OF)
    facts = [dict(t.split("=") for t in l.split()[2:]) for l in lines]
    for case, f in zip(CASES, facts):
        assert f["rows"] == iw.ROWS_OF[case], (case, f)
    assert {f["rows"] for f in facts} == ROW_KERNELS
    by = dict(zip(CASES, facts))
    # the surroundings the table of cases promises
    assert by[(400063, "m2=8,c=4")]["r5"] == "5" and by[(400063, "m2=8,c=4")]["cols"].startswith("radix5")
    assert by[(800283, "m2=4096,split5")]["split5"] == "1"
    assert by[(1200007, "m2=8192,c=2")]["c"] == "2"
    assert by[(127, None)]["m1"] == "1" and by[(127, None)]["m2"] == "4"           # n = 8
    assert (by[(196607, None)]["m1"], by[(196607, None)]["m2"]) == ("32", "128")


def test_every_case_has_room_for_the_summed_operand(shapes):
    for case, (n, q, c, sum_fast) in shapes.items():
        assert sum_fast == 1 and sum_product_ok(q, n, c), case
    n, q, _, _ = shapes[(196607, None)]
    assert n * (2**(q + 1) - 1) == 2**37 - 2**13          # n D = 2^37 (less n): the widest digits of the cases


def test_values_of_A_are_allowed_and_the_large_ones_are_used_somewhere(shapes):
    used = set()
    for case, (n, q, c, _) in shapes.items():
        values = iw.values_of_A(n, q)
        D = 2**(q + 1) - 1
        assert values[:2] == [1, 2**q - 1] and len(set(values)) == len(values), case
        for A in values:
            assert 0 < A < 2**32 and iw.allowed(A, n, q), (case, A)
            assert A * D <= n * D * D // 2                      # the rule as the issue states it
            assert 4 * (2 * A) * D < P                          # the doubled operand of mode 3, with the x4 of sum_product_ok's U, is a field element
        for A in (2**32 - 2, 2**32 - 1):
            assert (A in values) == (2 * A <= n * D), (case, A)
        used |= set(values)
    assert {2**32 - 2, 2**32 - 1} <= used
    assert 2**32 - 2 in iw.values_of_A(*shapes[(196607, None)][:2])      # the case the fused-sum failure is shown on
    assert iw.values_of_A(*shapes[(127, None)][:2]) == [1, 2**15 - 1]   # n = 8: no room for a 32-bit constant
    # allowed is a threshold in A
    n, q = shapes[(9941, "m2=64,c=8")][:2]
    top = n * (2**(q + 1) - 1) // 2
    assert iw.allowed(top, n, q) and not iw.allowed(top + 1, n, q)


def test_lift_patterns_cover_what_they_name():
    for n in (8, 512, 8192):
        for mask in (np.arange(n) % 2 == 0, (np.arange(n) // min(32, n // 2)) % 2 == 0):      # pairs; plane-major in runs of 64 words
            pats = dict(iw.lift_patterns(mask, 7))
            assert list(pats) == ["all", "plane-a", "plane-b", "word-0", "last-word", "one-in-64", "random-half"]
            assert pats["all"].all() and np.array_equal(pats["plane-a"], mask) and np.array_equal(pats["plane-b"], ~mask)
            assert np.flatnonzero(pats["word-0"]).tolist() == [0] and np.flatnonzero(pats["last-word"]).tolist() == [n - 1]
            one = pats["one-in-64"]
            assert int(one.sum()) == max(1, n // 64)
            if n >= 64:
                assert (one.reshape(-1, 64).sum(axis=1) == 1).all()              # one lane of every wave-sized run of words
                if n >= 128:
                    assert (one & mask).any() and (one & ~mask).any()
            half = pats["random-half"]
            assert 0 < int(half.sum()) < n
            if n >= 512:
                assert abs(int(half.sum()) - n // 2) < n // 8
            # on the image of a liftable constant every pattern lifts exactly the words it names
            for name, pat in pats.items():
                img = iw.constant_image(mask, 5, 0)
                assert iw.lift(img, pat) == int(pat.sum()), name
                assert np.array_equal(iw.fold(img), iw.constant_image(mask, 5, 0))
                assert np.array_equal(img >= U64(P), pat)
            # 2^32 - 1 has no second representative: only plane b moves
            img = iw.constant_image(mask, 2**32 - 1, 0)
            assert iw.lift(img, pats["all"]) == n // 2 and np.array_equal(img >= U64(P), ~mask)


def test_arbitrary_words_hold_every_edge_word_on_both_planes():
    for n in (8, 512, 8192):
        mask = np.arange(n) % 2 == 0
        seen = {True: set(), False: set()}
        for rot in range(12 if n < 48 else 1):
            R = iw.arbitrary_words(n, rot, 3)
            assert R.dtype == U64 and R.size == n
            for i in range(min(n, iw.EDGE_RUN)):
                assert int(R[i]) in EDGE_WORDS
                seen[bool(mask[i])].add(int(R[i]))
        assert seen[True] == seen[False] == set(EDGE_WORDS), n
        if n > iw.EDGE_RUN:
            tail = R[iw.EDGE_RUN:]
            assert len(set(tail.tolist())) == tail.size and (tail >= U64(P)).sum() <= 1      # uniform words: un-folded ones are rare


def test_mode3_generator_meets_the_classes_of_the_lazy_sum(shapes):
    """The arrays test_gpu_image_words.py loads for `mode 3, arbitrary words` (same generator, same seeds, its rotations and patterns; the
    plane mask of an engine replaced by two stand-ins), in both argument orders: at least one word pair with both words >= P, with
    fold(a) + b >= 2^64, with fold(a) + b in [P, 2^64), with the sum exactly P and with the sum exactly 0 -- per case, as the device
    self-test demands of its own operand list (selftest_cases.hpp GfLazySum)."""
    import test_gpu_image_words as g
    sizes = sorted({shapes[c][:2] for c in CASES})
    for n, q in sizes:
        for mask in (np.arange(n) % 2 == 0, (np.arange(n) // 32) % 2 == 0) if n >= 64 else (np.arange(n) % 2 == 0,):
            total = {}
            for A, rot, pname, R, S in g.arbitrary_pairs(n, q, mask):
                assert [(int(r) % P + int(s)) % P for r, s in zip(R[:200], S[:200])] == [A if m else 0 for m in mask[:200]]
                for a, b in ((R, S), (S, R)):
                    head = slice(0, 4 * iw.EDGE_RUN)         # the classes live among the edge words: count there, and in a sample of the rest
                    for k, v in iw.sum_classes(a[head], b[head]).items():
                        total[k] = total.get(k, 0) + v
                    got = iw.lazy_sum(a[head], b[head])
                    assert [v % P for v in got] == [A if m else 0 for m in mask[head]]
            for k in ("both>=P", "wraps", "lazy-sum", "sum==P", "sum==0"):
                assert total.get(k, 0) >= 1, (n, k, total)
