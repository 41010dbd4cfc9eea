"""The environment switches of the engine (README.md, "Switches": MI355_KERNELS, MI355_TUNE bits 0 and 5, MI355_HOST_CARRY) select kernels,
tile orders and the read-back path, never results: every setting -- alone and in every combination -- gives the oracle's digit vectors on
shapes of every kernel set ("combinations untested").  The switches are read when an engine is created.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import itertools

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

# exponent, plan: radix-8 columns + rows of 4096 (R = 2: the one shape whose front order bit 5 changes), rows of 2048 (one to a tile),
# radix-4 columns and rows (plane forms; the pair-form columns at 256 x 4096, the last entry), radix-5 columns of 1280 x 4 and 2560 x 2
# (bit 5), generic small tiles, runs of two digits (C = 1: the carry-fix path)
SHAPES = [(300007, "m2=8,c=4"), (300007, "m2=4096"), (1200007, "m2=2048,c=4"), (600011, "m2=2048"), (300007, "m2=1024"), (132049, "m2=16,c=4"),
          (800283, "m2=16,c=4"), (800283, "m2=8,c=2"), (9941, "m2=16,c=4"), (9941, "m2=128,c=2"), (521, "m2=8,c=2"), (127, "m2=2,c=1"),
          (30402457, "m2=4096")]

KERNELS = [None, "generic", "v2rows", "v2cols"]
TUNE = [0, 1, 32, 33]   # tile orders of the back (bit 0) and front (bit 5) sweeps
HOST_CARRY = [None, "1"]


def Engine(*a, **k):
    from prmers_amd import Engine as E
    return E(*a, **k)


def reference_run(p):
    """the oracle's digit vectors after a short chain that exercises every sweep variant: squarings with and without a factor, the LL
    step (sub borrows through the digits before the next squaring), a multiplicand image and a mul"""
    o = orc.Oracle(p, 3)
    rng = np.random.default_rng(p)
    x0 = int.from_bytes(rng.bytes((p + 7) // 8), "little") % ((1 << p) - 1)
    o.set_value(0, x0)
    out = []
    for a in (1, 3):
        o.square_mul(0, a)
    out.append(o.digits(0).copy())
    o.copy(1, 0); o.set_multiplicand(2, 1)
    o.sub(0, 2); o.square_mul(0); o.mul(0, 2)
    out.append(o.digits(0).copy())
    return x0, out, o.res64(0)


def engine_run(p, plan, x0):
    with Engine(p, 4, plan=plan) as e:
        e.set_int(0, x0)
        out = []
        for a in (1, 3):
            e.square_mul(0, a)
        out.append(e.digits(0).copy())
        e.copy(1, 0); e.set_multiplicand(2, 1)
        e.sub(0, 2); e.square_mul(0); e.mul(0, 2)
        out.append(e.digits(0).copy())
        return out, e.res64(0), e.describe()


@pytest.fixture(scope="module")
def refs():
    return {p: reference_run(p) for p in sorted({p for p, _ in SHAPES})}


def check(refs, p, plan, label):
    x0, want, r64 = refs[p]
    got, g64, desc = engine_run(p, plan, x0)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (p, plan, label, desc, i)
    assert g64 == r64, (p, plan, label)


def set_switches(monkeypatch, ks, tune, host):
    for name, value in (("MI355_KERNELS", ks), ("MI355_TUNE", tune), ("MI355_HOST_CARRY", host)):
        if value is None: monkeypatch.delenv(name, raising=False)
        else: monkeypatch.setenv(name, str(value))


@pytest.mark.parametrize("p,plan", SHAPES)
def test_every_switch_alone_gives_the_same_digits(p, plan, refs, monkeypatch):
    alone = [(None, None, None)] + [(ks, None, None) for ks in KERNELS[1:]] + [(None, t, None) for t in TUNE] + [(None, None, "1")]
    for ks, tune, host in alone:
        set_switches(monkeypatch, ks, tune, host)
        check(refs, p, plan, "kernels=%s tune=%s host_carry=%s" % (ks, tune, host))


@pytest.mark.parametrize("p,plan", SHAPES)
def test_switch_combinations_give_the_same_digits(p, plan, refs, monkeypatch):
    for ks, tune, host in itertools.product(KERNELS, TUNE, HOST_CARRY):
        set_switches(monkeypatch, ks, tune, host)
        check(refs, p, plan, "kernels=%s tune=%d host_carry=%s" % (ks, tune, host))
