"""Products of the second field family (GF(M61^2) x GF(M31^2): crt_kernels.hip, crt_rows.hpp, crt_carry.hpp, crt_engine.hip) at every
column length of the radix-8 kernel set, every class of the prime-factor index maps, and both ends of each size's exponent range
(crt_cases.py): seeded squarings and products with factor 2^32 - 1, a copied image, a subtraction between them -- against the libgmp
pins (golden/crt_product_pins.json) or Python integers, never against the engine's own carry -- then every digit at its maximum through
every kind of product against closed forms, and the composed operations on the three smallest sizes.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import time

import pytest

import crt_cases as cc

pytestmark = pytest.mark.gpu

RUNS = cc.runs()
COMPOSED = [(1, 12), (3, 12), (9, 12)]      # the smallest size of each radix: the radix-8 kernel set at H1 = 2


def CrtEngine(*a, **k):
    from prmers_amd import CrtEngine as E
    return E(*a, **k)


@pytest.mark.parametrize("odd,ln,which", RUNS, ids=["%s-%s" % (cc.case_id((o, l)), w) for o, l, w in RUNS])
def test_products_and_worst_case_digits(odd, ln, which):
    from test_gpu_operand_edges import _minus_one_words
    t0 = time.time()
    p, n = cc.exponent(odd, ln, which), odd << ln
    with CrtEngine(p, odd, n, reg_count=5) as e:
        cc.assert_engine(e, odd, ln)
        if odd > 1:
            assert e.algorithmic_bytes() == n * (8 + 8 + 96)      # back + carry in one kernel
        cc.product_script(e, odd, ln, which)
        cc.worst_case_script(e, odd, ln, which, _minus_one_words(e))
    print("crt products %s %s p=%d: %.2f s" % (cc.case_id((odd, ln)), which, p, time.time() - t0))


@pytest.mark.parametrize("odd,ln", COMPOSED, ids=[cc.case_id(c) for c in COMPOSED])
def test_composed_operations_on_the_radix8_kernel_set(odd, ln):
    """mul_add, mul_copy, square_mul_copy, exp_mul, square_mul_bits (the script of test_gpu_one_interface), mul_sum and
    square_mul_prepare (the second-family scripts of their own tests) at p_top, where every other test of them runs at p ~ 10^4 on the
    generic radix-2 kernels"""
    from test_gpu_mul_sum import mul_sum_script
    from test_gpu_one_interface import REGS, composed_script
    from test_gpu_square_prepare import square_prepare_script
    p, n = cc.p_top(odd, ln), odd << ln

    def make():
        e = CrtEngine(p, odd, n, reg_count=REGS)
        cc.assert_engine(e, odd, ln)
        return e
    composed_script(make, p)
    with make() as e:
        assert not e.mul_sum_is_fused() and not e.square_mul_prepare_is_fused()
        mul_sum_script(e, p)
        square_prepare_script(e, p)
