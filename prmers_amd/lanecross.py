"""The inverse of a register on every lane of an engine with lanes, with ONE inversion on the host whatever the lane count.

Lanes cannot talk to each other except through Engine.mul_sibling (include/mi355_lanecross.h): on every lane l,
dst[l] <- dst[l] * src[g] with g = ((l >> level) ^ 1) << level, the first lane of l's sibling block of 2^level lanes, where g is a lane,
and dst[l] * alt[l] where it is not (alt holds the image of 1).  That is enough for Montgomery's trick across the lanes:

    Up.    T <- copy(Z).  For s = 0 .. L - 1, L = levels(B):  R_s <- image of T,  mul_sibling(T, R_s, ONE, s).
           By induction T[l] after level s is the product of Z over l's block of 2^(s + 1) lanes, for EVERY l of the block: before level s
           every lane of a block of 2^s holds that block's product, so the sibling block's first lane holds the sibling's.  A sibling block
           is empty exactly when its first lane is >= B, and then the product by 1 is the right one.  After L levels every lane holds
           P = prod Z[l], for any B, a power of two or not.
    Once.  P is read from lane 0, u = P^-1 mod 2^p - 1 on the host (ecm.mod_inverse), u (or Mp - u) written to every lane of U.
    Down.  For every s: mul_sibling(U, R_s, ONE, s).  U[l] = u * prod_s R_s[sibling_s(l)], and the sibling blocks of l over all levels
           are exactly the lanes other than l, so U[l] = Z[l]^-1.

L prepares, 2 L sibling products, one copy, one lane read and one write; L + 2 registers beside Z and U (T, ONE and the R_s).  When P has no
inverse nothing is written: Z and U stay as they were and the caller gets gcd(P, Mp).  With one lane (L = 0) it is a copy, a read, an
inversion and a write.
"""
from .pm1 import big_gcd


def sibling(lane, level, lanes):
    """the lane whose image mul_sibling(.., level) gives lane `lane` of an engine with `lanes` lanes, None when it takes alt's"""
    g = ((lane >> level) ^ 1) << level
    return g if g < lanes else None


def levels(lanes):
    """L: levels of the up and of the down pass, ceil(log2 lanes)"""
    if lanes < 1:
        raise ValueError("lanes must be at least 1")
    return (lanes - 1).bit_length()


def registers_needed(lanes):
    """registers invert() wants beside Z and U: T, ONE and R_0 .. R_(L-1)"""
    return levels(lanes) + 2


def prepare_one(eng, one):
    """the image of 1 in register `one`, on every lane: once for any number of invert() calls that name it"""
    eng.set(one, 1)
    eng.set_multiplicand(one, one)


def invert(eng, z, u, work, negate=False, use_gmp=None, ops=None):
    """U[l] <- Z[l]^-1 mod 2^p - 1 on every lane (Mp - Z[l]^-1 when negate); Z stays as it is.
    eng: an engine with lanes and mul_sibling, or any object with one lane (no level, mul_sibling is not called).
    work: registers_needed(lanes) registers, (T, ONE, R_0, ..); ONE holds the image of 1 (prepare_one) and stays, the others are spent.
    ops: an object whose `prepares` and `products` are counted up (ecm._Ops).
    -> (True, 1), or (False, gcd(P, Mp)) when the product P of Z over the lanes has no inverse: then U was not written."""
    from .ecm import mod_inverse
    lanes = getattr(eng, "lanes", 1)
    L = levels(lanes)
    if len(work) < L + 2 or len({z, u, *work[:L + 2]}) != L + 4:
        raise ValueError("invert on %d lanes needs %d different work registers beside Z and U" % (lanes, L + 2))
    T, ONE, R = work[0], work[1], work[2:L + 2]
    mp = (1 << eng.p) - 1
    eng.copy(T, z)
    for s in range(L):
        eng.set_multiplicand(R[s], T)
        eng.mul_sibling(T, R[s], ONE, s)
    if ops is not None:
        ops.prepares += L
        ops.products += L
    P = eng.get_int(T, lane=0) if lanes > 1 else eng.get_int(T)
    inv = mod_inverse(P, mp, use_gmp) if P else 0
    if not inv:
        return False, (mp if P == 0 else big_gcd(P, mp, use_gmp))
    eng.set_int(u, mp - inv if negate else inv)          # every lane
    for s in range(L):
        eng.mul_sibling(u, R[s], ONE, s)
    if ops is not None:
        ops.products += L
    return True, 1
