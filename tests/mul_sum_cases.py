"""(exponent, plan) cases of the multiply-by-sum tests, shared by the GPU test and the host test that checks which kernels they reach."""
CASES = [
    (127, None), (521, "m2=4,c=2"), (9941, "m2=64,c=8"),
    (300007, "m2=1024"), (300007, "m2=2048"), (300007, "m2=4096"), (300007, "m2=8192"), (1200007, "m2=8192,c=2"),
    (400063, "m2=8,c=4"), (800283, "m2=4096,split5"),
    (19000013, "m2=1024"), (30402457, None),
    (204799, None), (196607, None),      # n = 8192 at its two largest digit widths: the first has no room for the summed operand (the two-product path)
]
ROW_KERNELS = {"generic", "radix4-pairs", "radix4-planes", "rows4096", "rows8192", "rows2048-one", "rows2048-two"}
FIELD = 2**64 - 2**32 + 1


def sum_product_ok(q, n, c):
    """plan.hpp sum_product_ok restated: the worst-case chain of fused_factor_ok at factor 1 with the convolution bound times 4: the
    summed multiplicand has digits up to 2 D (2 E once per run), and the weights leave a factor 2^c, c in {0, 1}, on every term of an
    unweighted coefficient"""
    D = 2**(q + 1) - 1
    runs = n // (2 * c)
    E = D
    for _ in range(64):
        U = 4 * ((n - runs) * D * D + runs * E * E if c >= 2 else n * D * D)
        if U >= FIELD:
            return False
        chi = U >> q
        carry = 0
        for _ in range(4096):
            r = D + carry + 2**32
            if r >= 2**64:
                return False
            nxt = (r >> q) + chi
            if nxt >= 2**64:
                return False
            if nxt == carry:
                break
            carry = nxt
        if c < 2:
            return True
        E2 = D + (carry >> (3 * q)) + 3
        if E2 >= 2**31:
            return False
        if E2 <= E:
            return True
        E = E2
    return False
