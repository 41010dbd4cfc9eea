"""The environment switches of the second field family (README.md, "Switches": MI355_CRT_KERNELS, MI355_CRT_TUNE bits 0 and 1,
MI355_HOST_CARRY) select kernels, tile orders and the read-back path, never results: all sixteen combinations of kernel set and tune bits
give the pinned (or integer) products at the top of every column length's exponent range -- each setting against the pins themselves,
not against the default run.  crt_cases.choose_kernels says which kernels a setting means; test_crt_cases.py checks that the matrix
reaches every one.  The switches are read when an engine is created.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import time

import pytest

import crt_cases as cc

pytestmark = pytest.mark.gpu

IDS = [cc.case_id(c) for c in cc.SWITCH_CASES]


def CrtEngine(*a, **k):
    from prmers_amd import CrtEngine as E
    return E(*a, **k)


def set_switches(monkeypatch, ks, tune, host):
    for name, value in (("MI355_CRT_KERNELS", ks), ("MI355_CRT_TUNE", tune), ("MI355_HOST_CARRY", host)):
        if value is None: monkeypatch.delenv(name, raising=False)
        else: monkeypatch.setenv(name, str(value))


def run(odd, ln, ks, tune, host):
    p, n = cc.p_top(odd, ln), odd << ln
    with CrtEngine(p, odd, n, reg_count=3) as e:
        cc.assert_engine(e, odd, ln, ks, tune or 0)
        cc.product_script(e, odd, ln, "top", with_copied_image=False, label="kernels=%s tune=%s host_carry=%s" % (ks, tune, host))


@pytest.mark.parametrize("ks", cc.KERNEL_SETS, ids=[k or "default" for k in cc.KERNEL_SETS])
@pytest.mark.parametrize("odd,ln", cc.SWITCH_CASES, ids=IDS)
def test_every_kernel_set_and_tune_setting_gives_the_pinned_products(odd, ln, ks, monkeypatch):
    t0 = time.time()
    for tune in cc.TUNES:
        set_switches(monkeypatch, ks, tune, None)
        run(odd, ln, ks, tune, None)
    print("crt switches %s kernels=%s: %.2f s" % (cc.case_id((odd, ln)), ks, time.time() - t0))


@pytest.mark.parametrize("odd,ln", cc.SWITCH_CASES, ids=IDS)
def test_no_switch_set_and_the_host_carry(odd, ln, monkeypatch):
    """nothing set at all (not even MI355_CRT_TUNE=0), and the host read-back and word-cutting paths on the default kernels"""
    for host in (None, "1"):
        set_switches(monkeypatch, None, None, host)
        run(odd, ln, None, None, host)
