"""The row kernels' modes 1 (mul, mul_add, mul_copy) and 3 (mul_sum) on multiplicand images whose 64-bit words the test writes itself
(tests/image_words.py): every representative of a word of GF(P) -- canonical, un-folded (w + P), 2^64 - 1 -- on every row kernel, against
Python integers.  An image that is A on plane a and 0 on plane b is the image of the integer A, so the expected product is A x mod
2^p - 1.  For dst = 1 the transformed residue is (1, 0) at every element, and the kernels compute gf::mul(1, y): for y in [P, 2^64) that
is the case "r >= P without carry" of dev::reduce_tail (gf.hpp), its slow branch, entered in every wave that holds such a word.
Every assertion names (p, plan, A, pattern, dst, operation).  Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

import image_words as iw
import orc
from image_words import CASES, CASE_IDS, P

pytestmark = pytest.mark.gpu

U64 = np.uint64
SEED = 64
REGS = 16
DST, IMG, IMG2, TMP, CPY, ZERO, AUX, AUX2, KEEP = 0, 1, 2, 3, 4, 5, 6, 7, 13    # registers; 8 .. 12 hold the dst values
FIRST_DST = 8


def rand_residue(rng, p):
    return int.from_bytes(rng.bytes((p + 7) // 8), "little") % ((1 << p) - 1)


def arbitrary_pairs(n, q, mask):
    """(A, rot, pattern name, R, S) of `mode 3, arbitrary words`: R arbitrary 64-bit words, S their complement to the image of A, lifted
    by a pattern.  A = 0 makes every sum = 0 (mod P), sums that are exactly P and exactly 0 among them.  (tests/test_image_words.py
    counts the word classes these arrays hold.)"""
    for A in (0, 2**q - 1):
        for rot in (range(12) if n < iw.EDGE_RUN else range(2)):      # a transform shorter than the edge run sees it over twelve calls
            R = iw.arbitrary_words(n, rot, SEED)
            pats = dict(iw.lift_patterns(mask, SEED + rot))
            for pname in ("none", "all", "random-half"):
                S = iw.complement(A, R, mask)
                if pname != "none":
                    iw.lift(S, pats[pname])
                yield A, rot, pname, R, S


class Case:
    def __init__(self, e, p, plan):
        self.e, self.p, self.plan, self.n, self.q, self.Mp = e, p, plan, e.n, p // e.n, (1 << p) - 1
        e.set(IMG, 1)
        e.set_multiplicand(IMG, IMG)
        self.one_words, self.tag = iw.split(e.get_data(IMG))
        assert self.one_words.size == self.n and int.from_bytes(self.tag, "little") & 1, self.where(1, "-", "-", "get_data of an image")
        self.mask = iw.plane_a(self.one_words)          # asserts: {w mod P} within {0, 1}, n/2 ones
        self.values = iw.values_of_A(self.n, self.q)
        self.patterns = iw.lift_patterns(self.mask, SEED)
        self.liftable = max(A for A in self.values if A < iw.LIFT_LIMIT)     # 2^32 - 2 (lift: 2^64 - 1) where the capacity admits it
        rng = np.random.default_rng([SEED, p])
        e.set(ZERO, 0)
        self.dsts = []
        for k, (name, v) in enumerate((("0", 0), ("1", 1), ("2", 2), ("2^p-2", self.Mp - 1), ("random-pending", None))):
            r = FIRST_DST + k
            if v is None:
                e.set_int(r, rand_residue(rng, p))
                e.square_mul(r, 3)                      # run carries pending
            else:
                e.set_int(r, v)
            e.copy(CPY, r)
            x = e.get_int(CPY)
            assert v is None or x == v
            self.dsts.append((name, r, x))
        self.y = rand_residue(rng, p)

    def red(self, v):
        return orc.mers_reduce(v, self.p)

    def where(self, A, pattern, dst, op):
        return "p=%d plan=%s A=%s pattern=%s dst=%s op=%s" % (self.p, self.plan, A if isinstance(A, str) else hex(A), pattern, dst, op)

    def load(self, reg, words, what=""):
        ok = self.e.set_data(reg, iw.join(words, self.tag))
        assert ok, "set_data refused a crafted image (%s): %s" % (what, self.e.L.mi355_engine_last_error().decode())

    def image(self, A, pattern=None):
        """the image of A, lifted where the pattern (a name of self.patterns) says"""
        w = iw.constant_image(self.mask, A, 0)
        if pattern not in (None, "none"):
            iw.lift(w, dict(self.patterns)[pattern])
        return w


@pytest.fixture(scope="module", params=CASES, ids=CASE_IDS)
def case(request):
    from prmers_amd import Engine
    p, plan = request.param
    with Engine(p, REGS, plan=plan) as e:
        yield Case(e, p, plan)


def test_image_of_one_is_one_on_plane_a_and_zero_on_plane_b(case):
    """the precondition of everything below, and the image of 1 written by the test multiplies like the engine's own"""
    c, e = case, case.e
    assert set(iw.fold(c.one_words).tolist()) == {0, 1} and int(c.mask.sum()) == c.n // 2, c.where(1, "-", "-", "set_multiplicand")
    assert np.array_equal(iw.constant_image(c.mask, 1, 0), iw.fold(c.one_words))
    assert c.values[:2] == [1, 2**c.q - 1] and all(iw.allowed(A, c.n, c.q) for A in c.values)
    c.load(IMG, c.image(1), "A=1")
    for name, r, x in c.dsts:
        e.copy(DST, r)
        e.mul(DST, IMG)
        assert e.get_int(DST) == x, c.where(1, "canonical", name, "mul")


def test_mode1_every_representative(case):
    c, e = case, case.e
    for A in c.values:
        base = c.image(A)
        c.load(IMG, base, hex(A))
        want, ref = {}, {}
        for name, r, x in c.dsts:
            for f in (1, 3):
                e.copy(DST, r)
                e.mul(DST, IMG, f)
                want[name, f] = c.red(f * A * x)
                assert e.get_int(DST) == want[name, f], c.where(A, "canonical", name, "mul f=%d" % f)
                ref[name, f] = e.digits(DST)
        for pname, pat in c.patterns:
            w = base.copy()
            lifted = iw.lift(w, pat)
            if lifted == 0:
                assert A == 2**32 - 1 and not (pat & ~c.mask).any(), c.where(A, pname, "-", "lift")     # only a pattern inside plane a of 2^32 - 1 lifts nothing
                continue
            assert int((w >= U64(P)).sum()) == lifted and np.array_equal(iw.fold(w), base)
            c.load(IMG, w, "%#x %s" % (A, pname))
            for name, r, x in c.dsts:
                for f in (1, 3):
                    e.copy(DST, r)
                    e.mul(DST, IMG, f)
                    assert np.array_equal(e.digits(DST), ref[name, f]), c.where(A, pname, name, "mul f=%d (digits against the un-lifted image)" % f)
                    assert e.get_int(DST) == want[name, f], c.where(A, pname, name, "mul f=%d" % f)


def test_mode1_mul_add_and_mul_copy_on_a_lifted_image(case):
    c, e = case, case.e
    A = c.liftable
    (_, radd, yadd), (name, r, x) = c.dsts[3], c.dsts[4]
    got = {}
    for pname in ("none", "all", "random-half"):
        c.load(IMG, c.image(A, pname), "%#x %s" % (A, pname))
        e.copy(DST, r)
        e.mul_add(DST, IMG, radd, 3)
        assert e.get_int(DST) == c.red(3 * A * x + yadd), c.where(A, pname, name, "mul_add f=3 add=2^p-2")
        d_add = e.digits(DST)
        e.copy(DST, r)
        e.set(CPY, 7)
        e.mul_copy(DST, IMG, CPY, 3)
        assert e.get_int(DST) == c.red(3 * A * x), c.where(A, pname, name, "mul_copy f=3")
        assert e.get_int(CPY) == c.red(3 * A * x) and e.is_equal(DST, CPY), c.where(A, pname, name, "mul_copy f=3 (the copy)")
        got[pname] = (d_add, e.digits(DST), e.digits(CPY))
    for pname in ("all", "random-half"):
        for k, op in enumerate(("mul_add", "mul_copy", "mul_copy (the copy)")):
            assert np.array_equal(got[pname][k], got["none"][k]), c.where(A, pname, name, op + " (digits against the un-lifted image)")


def test_mode3_constants(case):
    c, e = case, case.e
    assert e.mul_sum_is_fused() is True, c.where("-", "-", "-", "mul_sum_is_fused")      # no case may run two mode-1 products instead
    small, wide = c.values[0], c.values[1]
    pairs = [(small, wide), (wide, wide)]
    if 2**32 - 2 in c.values:
        pairs += [(2**32 - 2, 2**32 - 2), (2**32 - 2, small)]       # the first: 2^64 - 1 + 2^64 - 1 under ("all", "all")
    if 2**32 - 1 in c.values:
        pairs += [(2**32 - 1, 2**32 - 2)]
    lifts = [("all", "all"), ("all", "none"), ("none", "all"), ("plane-a", "plane-b"), ("one-in-64", "random-half"), ("random-half", "word-0"),
             ("last-word", "all")]
    for A1, A2 in pairs:
        for p1, p2 in lifts:
            c.load(IMG, c.image(A1, p1), "%#x %s" % (A1, p1))
            c.load(IMG2, c.image(A2, p2), "%#x %s" % (A2, p2))
            for name, r, x in c.dsts:
                want = c.red((A1 + A2) * x)
                for a, b, order in ((IMG, IMG2, "a+b"), (IMG2, IMG, "b+a")):
                    e.copy(DST, r)
                    e.mul_sum(DST, a, b, TMP)
                    assert e.get_int(DST) == want, c.where("%#x+%#x" % (A1, A2), p1 + "|" + p2, name, "mul_sum " + order)
        # the same image as both sources
        for pname in ("all", "random-half", "none"):
            c.load(IMG, c.image(A1, pname), "%#x %s" % (A1, pname))
            for name, r, x in c.dsts:
                e.copy(DST, r)
                e.mul_sum(DST, IMG, IMG, TMP)
                assert e.get_int(DST) == c.red(2 * A1 * x), c.where("%#x twice" % A1, pname, name, "mul_sum same image")


def test_mode3_arbitrary_words(case):
    """Y = arbitrary words, Y2 = their complement to the image of A: the sum is taken word by word, so any wrong index on either
    image (a partner plane read from the wrong place) leaves a word that is not A or 0"""
    c, e = case, case.e
    assert e.mul_sum_is_fused() is True, c.where("-", "-", "-", "mul_sum_is_fused")
    for A, rot, pname, R, S in arbitrary_pairs(c.n, c.q, c.mask):
        assert np.array_equal(iw.fold(iw.as_words(iw.lazy_sum(R[:64], S[:64]))), iw.constant_image(c.mask, A, 0)[:64])
        c.load(IMG, R, "arbitrary words rot=%d" % rot)
        c.load(IMG2, S, "complement %s" % pname)
        for name, r, x in c.dsts[1:]:
            for a, b, order in ((IMG, IMG2, "R+S"), (IMG2, IMG, "S+R")):
                e.copy(DST, r)
                e.mul_sum(DST, a, b, TMP)
                where = c.where(A, "rot=%d complement=%s" % (rot, pname), name, "mul_sum " + order)
                assert e.get_int(DST) == c.red(A * x), where
                if A == 0:
                    assert e.is_equal(DST, ZERO), where


def test_mode3_a_real_image_plus_a_crafted_one(case):
    c, e = case, case.e
    assert e.mul_sum_is_fused() is True, c.where("-", "-", "-", "mul_sum_is_fused")
    A = c.liftable
    e.set_int(AUX, c.y)
    e.set_multiplicand(IMG2, AUX)
    for pname in ("all", "random-half", "plane-b"):
        c.load(IMG, c.image(A, pname), "%#x %s" % (A, pname))
        for name, r, x in c.dsts[1:]:
            e.copy(AUX, r); e.mul(AUX, IMG2)
            e.copy(AUX2, r); e.mul(AUX2, IMG)
            e.add(AUX, AUX2)
            parts = e.digits(AUX)
            for a, b, order in ((IMG2, IMG, "y+A"), (IMG, IMG2, "A+y")):
                e.copy(DST, r)
                e.mul_sum(DST, a, b, TMP)
                where = c.where(A, pname, name, "mul_sum %s, y a real image" % order)
                assert np.array_equal(e.digits(DST), parts), where + " (digits against mul, mul, add)"
                if c.p <= 400063:
                    assert e.get_int(DST) == c.red(x * (c.y + A)), where


def test_real_images_do_not_depend_on_the_representative(case, record_property):
    """set_multiplicand (mode 2) and square_mul_prepare (mode 4) store the same words mod P; the folded words multiply like the stored
    ones.  How many stored words were un-folded is printed and recorded (zero is a legitimate answer)."""
    c, e = case, case.e
    name, r, x = c.dsts[4]
    e.set_int(AUX, c.y)
    e.square_mul(AUX, 3)                        # run carries pending on the register both images are taken from
    e.copy(AUX2, AUX)
    e.copy(CPY, AUX)
    y = e.get_int(CPY)
    e.copy(TMP, AUX)
    e.square_mul(TMP)
    e.set_multiplicand(IMG, AUX)
    e.square_mul_prepare(AUX2, IMG2, 1)
    w2, tag2 = iw.split(e.get_data(IMG))
    w4, tag4 = iw.split(e.get_data(IMG2))
    assert tag2 == tag4 == c.tag
    assert np.array_equal(iw.fold(w2), iw.fold(w4)), c.where("-", "-", "-", "set_multiplicand against square_mul_prepare, words mod P")
    assert np.array_equal(e.digits(AUX2), e.digits(TMP)), c.where("-", "-", "-", "square_mul_prepare (the square, against square_mul)")
    if c.p <= 400063:                           # (a product of two full residues in Python: seconds at the largest exponents)
        assert e.get_int(AUX2) == c.red(y * y), c.where("-", "-", "-", "square_mul_prepare (the square)")
    lazy2, lazy4 = int((w2 >= U64(P)).sum()), int((w4 >= U64(P)).sum())
    print("\nun-folded image words: p=%d plan=%s rows=%s n=%d set_multiplicand=%d square_mul_prepare=%d (prepare fused: %s)"
          % (c.p, c.plan, iw.ROWS_OF[c.p, c.plan], c.n, lazy2, lazy4, e.square_mul_prepare_is_fused()))
    record_property("unfolded_words", "%s n=%d mode2=%d mode4=%d" % (iw.ROWS_OF[c.p, c.plan], c.n, lazy2, lazy4))
    e.copy(DST, r)
    e.mul(DST, IMG)
    stored = e.digits(DST)
    if c.p <= 400063:
        assert e.get_int(DST) == c.red(x * y), c.where("y", "as stored", name, "mul")
    for words, what in ((iw.fold(w2), "folded"), (w4, "as stored by square_mul_prepare")):
        c.load(IMG, words, what)
        e.copy(DST, r)
        e.mul(DST, IMG)
        assert np.array_equal(e.digits(DST), stored), c.where("y", what, name, "mul")


def test_set_data_of_a_crafted_image_changes_nothing_else(case):
    c, e = case, case.e
    A = c.liftable
    held = [ZERO, KEEP] + [r for _, r, _ in c.dsts]          # the registers the other tests of the case rely on keep what they hold
    others = [r for r in range(REGS) if r not in [IMG, IMG2] + held]
    for r in others:
        e.set_int(r, 0x5EED0000 + r)

    def dst_values():
        out = [e.get_int(ZERO)]
        for _, r, _ in c.dsts:
            e.copy(KEEP, r)
            out.append(e.get_int(KEEP))
        return out
    first = iw.join(c.image(A, "random-half"), c.tag)
    second = iw.join(c.image(c.values[0], "all"), c.tag)
    assert e.set_data(IMG2, second) and e.set_data(IMG, first)
    assert [e.get_int(r) for r in others] == [0x5EED0000 + r for r in others], c.where(A, "random-half", "-", "set_data")
    assert dst_values() == [0] + [x for _, _, x in c.dsts], c.where(A, "random-half", "-", "set_data")
    e.set_int(DST, 0x5EED)
    e.mul(DST, IMG2)                            # the image loaded first still multiplies
    assert e.get_int(DST) == c.red(0x5EED * c.values[0]), c.where(c.values[0], "all", "0x5eed", "mul after set_data of another register")
    # the sources are intact after mul_sum: byte for byte, and they multiply again
    name, r, x = c.dsts[4]
    e.copy(DST, r)
    e.mul_sum(DST, IMG, IMG2, TMP)
    assert e.get_int(DST) == c.red((A + c.values[0]) * x), c.where(A, "random-half|all", name, "mul_sum")
    assert np.array_equal(e.get_data(IMG), first) and np.array_equal(e.get_data(IMG2), second), c.where(A, "random-half|all", name, "sources after mul_sum")
    e.mul(DST, IMG)
    e.mul(DST, IMG2)
    assert e.get_int(DST) == c.red((A + c.values[0]) * x * A * c.values[0]), c.where(A, "random-half|all", name, "mul by the sources after mul_sum")
    others = [r for r in others if r not in (DST, TMP)]
    assert [e.get_int(r) for r in others] == [0x5EED0000 + r for r in others], c.where(A, "random-half|all", "-", "registers after mul_sum")
    assert dst_values() == [0] + [x for _, _, x in c.dsts], c.where(A, "random-half|all", "-", "registers after mul_sum")
