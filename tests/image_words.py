"""Crafted multiplicand images: the 64-bit words of a raw image (Engine.get_data / set_data) written by the test itself, so that the row
kernels' modes 1 and 3 meet every representative of a word of GF(P), P = 2^64 - 2^32 + 1, and the expected product is a plain integer.
Shared by tests/test_image_words.py (no GPU) and tests/test_gpu_image_words.py; imports nothing that needs a GPU.

The construction.  Digit 0 has weight 1, the pair transform of a delta at pair 0 is constant and the four-step twiddle of column 0 is 1,
so the image of the value 1 is, mod P, the word 1 on plane a and 0 on plane b of every pair -- in every kernel's private order of the
words.  The positions of the ones are therefore the plane-a mask of the engine (plane_a), with no knowledge of a layout.  By linearity
an image that is A on plane a and 0 on plane b is the image of the integer A: mul(dst, image) gives A x mod 2^p - 1 for dst = x.  A need
not fit digit 0; the product is exact while allowed(A, n, q) holds."""
import numpy as np

P = 2**64 - 2**32 + 1
U64 = np.uint64
_P = U64(P)
LIFT_LIMIT = 2**32 - 1          # a canonical word w has a second 64-bit representative w + P exactly when w < 2^64 - P = 2^32 - 1

EDGE_WORDS = [0, 1, 2**32 - 2, 2**32 - 1, 2**32, 2**63, P - 1, P, P + 1, 2**64 - 2**32, 2**64 - 2, 2**64 - 1]

# (exponent, plan) and the row kernel the case must reach (plan.hpp choose_kernels; tests/test_image_words.py checks it with
# tests/host/plan_query.cpp): the smallest shapes of tests/mul_sum_cases.py that reach each of the seven kernels, plus the generic rows
# under radix-5 columns, rows of 4096 under split columns and rows of 8192 with runs of two pairs.  Every one has room for a summed operand.
CASES = [
    (127, None), (9941, "m2=64,c=8"), (196607, None), (400063, "m2=8,c=4"),
    (300007, "m2=1024"), (19000013, "m2=1024"), (300007, "m2=2048"), (30402457, None),
    (300007, "m2=4096"), (800283, "m2=4096,split5"), (300007, "m2=8192"), (1200007, "m2=8192,c=2"),
]
ROWS_OF = {
    (127, None): "generic", (9941, "m2=64,c=8"): "generic", (196607, None): "generic", (400063, "m2=8,c=4"): "generic",
    (300007, "m2=1024"): "radix4-planes", (19000013, "m2=1024"): "radix4-pairs", (300007, "m2=2048"): "rows2048-one",
    (30402457, None): "rows2048-two", (300007, "m2=4096"): "rows4096", (800283, "m2=4096,split5"): "rows4096",
    (300007, "m2=8192"): "rows8192", (1200007, "m2=8192,c=2"): "rows8192",
}
CASE_IDS = ["%d-%s" % (p, s or "default") for p, s in CASES]


# ---- raw buffers ---------------------------------------------------------------------------------------------------------------

def split(buf):
    """get_data buffer -> (the n words of the register as uint64, little endian; the 8 bytes of the tag)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    assert buf.size % 8 == 0 and buf.size >= 16
    return np.frombuffer(buf[:-8].tobytes(), dtype="<u8").astype(U64), buf[-8:].tobytes()


def join(words, tag):
    """the buffer set_data takes: the words, then the tag they were read with"""
    words = np.ascontiguousarray(words, dtype=U64)
    assert len(tag) == 8
    return np.concatenate([np.frombuffer(words.astype("<u8").tobytes(), dtype=np.uint8), np.frombuffer(tag, dtype=np.uint8)])


# ---- words ---------------------------------------------------------------------------------------------------------------------

def as_words(v, n=None):
    """Python integers in [0, 2^64) (or an array) as uint64 words"""
    a = np.array(v, dtype=U64) if not isinstance(v, np.ndarray) else v.astype(U64)
    return a if n is None else np.broadcast_to(a, (n,)).copy()


def fold(words):
    """w mod P: w - P where w >= P (2^64 < 2 P, so one subtraction)"""
    w = as_words(words)
    return np.where(w >= _P, w - _P, w)


def lift(words, mask):
    """In place: the words under `mask` whose canonical value is below 2^32 - 1 become that value + P (the other representative, at
    most 2^64 - 1); every other word stays.  Returns the number of words lifted."""
    assert words.dtype == U64 and mask.dtype == np.bool_ and words.shape == mask.shape
    c = fold(words)
    sel = mask & (c < U64(LIFT_LIMIT))
    words[sel] = c[sel] + _P           # < 2^32 - 1 + P = 2^64: never wraps
    return int(sel.sum())


def plane_a(words_of_image_of_1):
    """The plane-a mask of an engine from the words of its image of the value 1: mod P they are 0 or 1, with n/2 ones."""
    w = fold(words_of_image_of_1)
    other = w[(w != U64(0)) & (w != U64(1))]
    assert other.size == 0, "the image of 1 holds %d words that are neither 0 nor 1 mod P, the first %#x" % (other.size, int(other[0]))
    mask = w == U64(1)
    assert 2 * int(mask.sum()) == w.size, "the image of 1 has %d ones among %d words" % (int(mask.sum()), w.size)
    return mask


def constant_image(mask, ra, rb):
    """words ra on plane a and rb on plane b; each a Python integer in [0, 2^64) or an array of one word per position"""
    n = mask.size
    return np.where(mask, as_words(ra, n), as_words(rb, n))


def complement(A, R, mask):
    """For arbitrary 64-bit words R the canonical words S with fold(R) + S = A (mod P) on plane a and = 0 on plane b: A - fold(R), or
    A + (P - fold(R)) when fold(R) > A (below P, since P - fold(R) < P - A)."""
    assert 0 <= A < 2**32
    f = fold(R)
    t = np.where(mask, U64(A), U64(0))
    big = f > t
    return np.where(big, t + (_P - f), t - np.where(big, U64(0), f))


# ---- capacity and the values of A ------------------------------------------------------------------------------------------------

def allowed(A, n, q):
    """The product by the image of A is exact: its unweighted coefficients are A x_k (digit 0 has weight 1), at most A D with
    D = 2^(q+1) - 1 the largest digit, against n D^2 for an ordinary product of n digits -- kept a factor 2 below that.  (The plan's own
    bound carries a further factor 2 for the weights; a pending run carry adds a few units to one digit of a run.)  Mode 3 sums two such
    images: 2 A D <= n D^2, inside the x4 of plan.hpp sum_product_ok, which every case here passes."""
    D = 2**(q + 1) - 1
    return 2 * A * D <= n * D * D


def values_of_A(n, q):
    """1, the largest value of a narrow digit, and where the capacity admits them 2^32 - 2 (whose lift is 2^64 - 1) and 2^32 - 1 (the
    largest canonical word without a second representative)"""
    return [1, 2**q - 1] + [A for A in (2**32 - 2, 2**32 - 1) if allowed(A, n, q)]


# ---- lift patterns -----------------------------------------------------------------------------------------------------------------

def lift_patterns(mask, seed):
    """[(name, positions)]: which words of an image are lifted"""
    n = mask.size
    i = np.arange(n)
    one = lambda k: i == k
    rng = np.random.default_rng([seed, n])
    return [("all", np.ones(n, dtype=bool)), ("plane-a", mask.copy()), ("plane-b", ~mask), ("word-0", one(0)), ("last-word", one(n - 1)),
            # one word of every 64 (n < 64: one word), at a position that moves by 37 from block to block: every lane over 64 blocks,
            # both halves of a run of 64 within two
            ("one-in-64", i % 64 == (37 * (i // 64) + 5) % min(64, n)), ("random-half", rng.random(n) < 0.5)]


# ---- mode 3: arbitrary words ---------------------------------------------------------------------------------------------------------

EDGE_RUN = 4 * len(EDGE_WORDS)


def arbitrary_words(n, rot, seed):
    """R: EDGE_WORDS cycled over the first words (at most four cycles, each shifted by one against the one before, so that an edge word
    meets both planes; `rot` shifts them all: small transforms see every edge word over a few calls), seeded uniform 64-bit words after."""
    rng = np.random.default_rng([seed, n, rot])
    R = rng.integers(0, 2**64, size=n, dtype=U64)
    k = np.arange(min(n, EDGE_RUN))
    R[:k.size] = np.array(EDGE_WORDS, dtype=U64)[(k + k // len(EDGE_WORDS) + rot) % len(EDGE_WORDS)]
    return R


def sum_classes(a, b):
    """What gf::add_lazy_any(a, b) = add_lazy(fold(a), b) meets, word by word: counts of the classes the self-test's rule names."""
    a, b = as_words(a), as_words(b)
    fa = [int(v) for v in fold(a)]
    bi = [int(v) for v in b]
    ai = [int(v) for v in a]
    s = [x + y for x, y in zip(fa, bi)]
    return {
        "both>=P": sum(1 for x, y in zip(ai, bi) if x >= P and y >= P),
        "wraps": sum(1 for v in s if v >= 2**64),
        "lazy-sum": sum(1 for v in s if P <= v < 2**64),
        "sum==P": sum(1 for v in s if v == P),
        "sum==0": sum(1 for v in s if v == 0),
    }


def lazy_sum(a, b):
    """gf::add_lazy_any word by word in Python integers (gf.hpp): fold a, add, fold one carry with 2^64 = 2^32 - 1"""
    out = []
    for x, y in zip(as_words(a).tolist(), as_words(b).tolist()):
        s = (x - P if x >= P else x) + y
        out.append(s - 2**64 + 2**32 - 1 if s >= 2**64 else s)
    return out
