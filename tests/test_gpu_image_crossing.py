"""Raw register images (get_data / set_data / get_checkpoint / set_checkpoint) read by ANOTHER engine.  The rule: set_data and
set_checkpoint either restore exactly the value that was written or return false; they never load something else.  The size of an image
is the same for every plan of an exponent (8 n + 8 bytes), so its last word carries a fingerprint of the layout (plan.hpp register_tag):
digits lie in tile-major order, a function of (M1, M2, C, split5); a multiplicand image is in the form of the row kernel that wrote it,
with its rows in the order of the column kernels' frequency labels.  Switches that leave the layout alone must keep loading.
Every value read is compared with Python integers.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import itertools

import numpy as np
import pytest

import crt_cases as cc
import orc

pytestmark = pytest.mark.gpu

P = 300007
MP = (1 << P) - 1
PLANS = {"m2=4096": "marin-hip:n=16384:m1=2:m2=4096:c=16", "m2=8,c=4": "marin-hip:n=16384:m1=1024:m2=8:c=4",
         "m2=1024": "marin-hip:n=16384:m1=8:m2=1024:c=4", None: "marin-hip:n=16384:m1=32:m2=256:c=4"}
SWITCHES = ("MI355_KERNELS", "MI355_TUNE", "MI355_HOST_CARRY", "MI355_CRT_KERNELS", "MI355_CRT_TUNE")
SENTINEL = 0x5EED5EED5EED


def residue(seed, p=P):
    rng = np.random.default_rng([p, seed])
    return int.from_bytes(rng.bytes((p + 7) // 8), "little") % ((1 << p) - 1)


def red(v, p=P):
    return orc.mers_reduce(v + ((1 << p) - 1) if v < 0 else v, p)


X, V, W = residue(1), residue(2), residue(3)
V2 = red(red(V * V) - 2)             # register 1: written with run carries pending and a subtraction borrowed through the digits
XW = red(X * W)


def set_switches(monkeypatch, **values):
    for name in SWITCHES:
        if name in values: monkeypatch.setenv(name, str(values[name]))
        else: monkeypatch.delenv(name, raising=False)


def engine(plan):
    from prmers_amd import Engine
    e = Engine(P, 4, plan=plan)
    assert e.describe() == PLANS[plan], (plan, e.describe())
    return e


def write(plan):
    """{register name: image} and the checkpoint of an engine of `plan` under the current switches: X, V^2 - 2, the image of W, zero"""
    with engine(plan) as e:
        e.set_int(0, X)
        e.set_int(1, V)
        e.square_mul(1)
        e.sub(1, 2)
        e.set_int(2, W)
        e.set_multiplicand(2, 2)
        out = {"digits": e.get_data(0), "carried": e.get_data(1), "image": e.get_data(2), "checkpoint": e.get_checkpoint()}
        assert e.get_int(1) == V2            # (reading the image left the register as it was)
        return out


def loads(e, img):
    """the three registers load into e and read back as written; the image multiplies"""
    assert e.set_data(0, img["digits"]) and e.get_int(0) == X
    assert e.set_data(1, img["carried"]) and e.get_int(1) == V2
    e.square_mul(1)
    assert e.get_int(1) == red(V2 * V2)      # and it is a residue the engine can go on with
    image_loads(e, img)
    e.set_int(0, SENTINEL)
    assert e.set_checkpoint(img["checkpoint"])
    assert (e.get_int(0), e.get_int(1), e.get_int(3)) == (X, V2, 0)
    e.mul(0, 2)
    assert e.get_int(0) == XW


def image_loads(e, img):
    assert e.set_data(2, img["image"])
    e.set_int(0, X)
    e.mul(0, 2)
    assert e.get_int(0) == XW
    with pytest.raises(Exception, match="multiplicand"):
        e.square_mul(2)


def refuses(e, img, names=("digits", "carried", "image")):
    """nothing of img loads into e, and every register stays as it was"""
    for r in range(3):
        e.set_int(r, SENTINEL + r)
    for r, name in enumerate(("digits", "carried", "image")):
        if name in names:
            assert not e.set_data(r, img[name]), name
            assert not e.set_data(3, img[name]), name
    if "checkpoint" in img and len(names) == 3:
        assert not e.set_checkpoint(img["checkpoint"])
    assert [e.get_int(r) for r in range(4)] == [SENTINEL, SENTINEL + 1, SENTINEL + 2, 0]
    e.square_mul(0)
    assert e.get_int(0) == red(SENTINEL * SENTINEL)


@pytest.mark.parametrize("src", list(PLANS), ids=[k or "default" for k in PLANS])
def test_between_plans_of_one_exponent(src, monkeypatch):
    """every ordered pair of four plans: the writer's own plan loads, every other plan refuses -- digits, a register written with pending
    carries, a multiplicand image and the whole checkpoint"""
    set_switches(monkeypatch)
    img = write(src)
    assert len({PLANS[k] for k in PLANS}) == 4
    for dst in PLANS:
        with engine(dst) as e:
            assert e.get_register_data_size() == img["digits"].size == 8 * 16384 + 8      # the size says nothing about the plan
            if dst == src:
                loads(e, img)
            else:
                refuses(e, img)


def test_an_image_without_a_fingerprint_or_of_another_exponent_is_refused(monkeypatch):
    set_switches(monkeypatch)
    img = write("m2=4096")
    from prmers_amd import Engine
    with engine("m2=4096") as e:
        for name, kind in (("digits", 0), ("image", 1)):
            bare = img[name].copy()
            bare[-8:] = np.frombuffer(np.uint64(kind).tobytes(), dtype=np.uint8)     # the tag of earlier versions: the kind alone
            e.set_int(0, SENTINEL)
            assert not e.set_data(0, bare)
            flipped = img[name].copy()
            flipped[-1] ^= 0x40
            assert not e.set_data(0, flipped)
            assert e.get_int(0) == SENTINEL
    with Engine(301447, 4, plan="m2=4096") as e:      # the same transform size and plan, another exponent: other digit widths
        assert e.describe() == PLANS["m2=4096"] and e.get_register_data_size() == img["digits"].size
        e.set_int(0, SENTINEL)
        assert not e.set_data(0, img["digits"]) and not e.set_data(1, img["image"]) and not e.set_checkpoint(img["checkpoint"])
        assert e.get_int(0) == SENTINEL and e.get_int(1) == 0


# MI355_KERNELS -> (column kernels, row kernel) of an engine of the plan (tests/test_host_logic.py pins these against plan.hpp
# choose_kernels).  The row kernel defines the form of an image's words.  The column kernels define the order of its rows, which is
# bit-reversed for every column kernel of a power-of-two transform: at m2=8,c=4 the radix-8 and the generic columns exchange images.
KERNELS_OF = {
    "m2=4096": {None: ("generic", "rows4096"), "v2rows": ("generic", "rows4096"), "v2cols": ("generic", "generic"), "generic": ("generic", "generic")},
    "m2=8,c=4": {None: ("radix8-1024", "generic"), "v2cols": ("radix8-1024", "generic"), "v2rows": ("generic", "generic"), "generic": ("generic", "generic")},
}


def image_form(plan, kernels):
    return KERNELS_OF[plan][kernels][1]


@pytest.mark.parametrize("plan", list(KERNELS_OF))
def test_switches_on_one_plan(plan, monkeypatch):
    """MI355_TUNE and MI355_HOST_CARRY change no stored word: everything keeps loading, both ways.  MI355_KERNELS leaves the digits
    where they are, so residues keep loading; a multiplicand image loads where its form is the same and is refused elsewhere
    (default kernels to v2cols and back at m2=4096: same layout, but generic rows against the rows of 4096)"""
    settings = [{}, {"MI355_TUNE": 33}, {"MI355_TUNE": 1}, {"MI355_TUNE": 32}, {"MI355_HOST_CARRY": 1}, {"MI355_KERNELS": "generic"},
                {"MI355_KERNELS": "v2rows"}, {"MI355_KERNELS": "v2cols"}]
    images = []
    for s in settings:
        set_switches(monkeypatch, **s)
        images.append(write(plan))
    for (si, src), (di, dst) in itertools.permutations(enumerate(settings), 2):
        if src and dst:
            continue                       # every setting against the default, both ways
        set_switches(monkeypatch, **dst)
        same = image_form(plan, src.get("MI355_KERNELS")) == image_form(plan, dst.get("MI355_KERNELS"))
        with engine(plan) as e:
            if same:
                loads(e, images[si])
            else:
                refuses(e, images[si], names=("image",))
                assert not e.set_checkpoint(images[si]["checkpoint"])          # (register 2 of the checkpoint is that image)
                assert e.set_data(0, images[si]["digits"]) and e.get_int(0) == X
                assert e.set_data(1, images[si]["carried"]) and e.get_int(1) == V2


def test_image_between_kernel_sets_that_differ_in_rows_only(monkeypatch):
    """generic and v2cols run the same kernels at m2=4096, v2rows and the default too: those pairs exchange images"""
    for a, b in (("generic", "v2cols"), ("v2cols", "generic"), ("v2rows", None), (None, "v2rows")):
        set_switches(monkeypatch, **({"MI355_KERNELS": a} if a else {}))
        img = write("m2=4096")
        set_switches(monkeypatch, **({"MI355_KERNELS": b} if b else {}))
        with engine("m2=4096") as e:
            image_loads(e, img)


def test_radix5_image_between_column_kernels(monkeypatch):
    """with a radix-5 stage the column kernels number the rows of the work buffer each in their own way (prime-factor labels): columns
    of 1280 x 4 run on the radix-5 kernels by default and under v2cols, on the generic ones under v2rows and `generic`, all with generic
    rows.  An image crosses inside each class and is refused between them; residues cross everywhere."""
    from prmers_amd import Engine
    p, text = 400063, "marin-hip:n=20480:m1=1280:m2=8:c=4"
    x, w = residue(7, p), residue(8, p)
    cols = {None: "radix5-1280", "v2cols": "radix5-1280", "v2rows": "generic", "generic": "generic"}

    def make():
        e = Engine(p, 3, plan="m2=8,c=4")
        assert e.describe() == text
        return e
    written = {}
    for ks in cols:
        set_switches(monkeypatch, **({"MI355_KERNELS": ks} if ks else {}))
        with make() as e:
            e.set_int(0, x)
            e.set_int(1, w)
            e.set_multiplicand(1, 1)
            written[ks] = (e.get_data(0), e.get_data(1))
    for src, dst in itertools.permutations(cols, 2):
        set_switches(monkeypatch, **({"MI355_KERNELS": dst} if dst else {}))
        with make() as e:
            assert e.set_data(0, written[src][0]) and e.get_int(0) == x
            e.set_int(1, SENTINEL)
            if cols[src] == cols[dst]:
                assert e.set_data(1, written[src][1])
                e.mul(0, 1)
                assert e.get_int(0) == red(x * w, p), (src, dst)
            else:
                assert not e.set_data(1, written[src][1]) and e.get_int(1) == SENTINEL, (src, dst)


# ---- the two families, and the second family's own switches --------------------------------------------------------------------

Q = 9941
CRT_TEXT = "crt-hip:n=288:odd=9:m=32:h1=1:h2=16:generic"


def test_goldilocks_and_crt_images_do_not_cross(monkeypatch):
    set_switches(monkeypatch)
    from prmers_amd import CrtEngine, Engine
    x = residue(4, Q)
    with Engine(Q, 4) as g, CrtEngine(Q, 9, reg_count=4) as c:
        assert g.describe() == "marin-hip:n=512:m1=8:m2=32:c=4" and c.describe() == CRT_TEXT
        assert g.get_register_data_size() == 8 * 512 + 8 and c.get_register_data_size() == 12 * 288 + 8
        g.set_int(0, x); c.set_int(0, x)
        g.set_int(1, SENTINEL); c.set_int(1, SENTINEL)
        assert not c.set_data(1, g.get_data(0)) and not g.set_data(1, c.get_data(0))
        assert not c.set_checkpoint(g.get_checkpoint()) and not g.set_checkpoint(c.get_checkpoint())
        assert g.get_int(1) == SENTINEL and c.get_int(1) == SENTINEL
        assert g.set_data(1, g.get_data(0)) and c.set_data(1, c.get_data(0))
        assert g.get_int(1) == x and c.get_int(1) == x


def crt_write(p, odd, n=0):
    from prmers_amd import CrtEngine
    x, w = residue(5, p), residue(6, p)
    with CrtEngine(p, odd, n, reg_count=3) as e:
        e.set_int(0, x)
        e.square_mul(0, 3)                   # weakly carried digits
        e.set_int(1, w)
        e.set_multiplicand(1, 1)
        return {"text": e.describe(), "digits": e.get_data(0), "image": e.get_data(1), "x": red(3 * x * x, p), "w": w}


def crt_loads(e, img, p, image=True):
    assert e.set_data(0, img["digits"]) and e.get_int(0) == img["x"]
    if image:
        assert e.set_data(1, img["image"])
        e.mul(0, 1)
        assert e.get_int(0) == red(img["x"] * img["w"], p)


def test_second_family_across_its_kernel_sets(monkeypatch):
    """a residue is in natural order under every MI355_CRT_KERNELS setting and loads.  At 9941 (rows of 16) every setting runs the
    generic passes (the plan text says so), so an image crosses too; at 9 x 2^12 the default runs the radix-8 row kernel, whose packed
    spectrum is its own form: an image between it and `generic` is refused, between the settings that keep the radix-8 rows it loads."""
    from prmers_amd import CrtEngine
    written = {}
    for ks in cc.KERNEL_SETS:
        set_switches(monkeypatch, **({"MI355_CRT_KERNELS": ks} if ks else {}))
        written[ks] = crt_write(Q, 9)
        assert written[ks]["text"] == CRT_TEXT
    for src, dst in itertools.permutations(cc.KERNEL_SETS, 2):
        set_switches(monkeypatch, **({"MI355_CRT_KERNELS": dst} if dst else {}))
        with CrtEngine(Q, 9, reg_count=3) as e:
            crt_loads(e, written[src], Q)
    p, n = cc.p_low(9, 12), 9 << 12
    for ks in cc.KERNEL_SETS:
        set_switches(monkeypatch, **({"MI355_CRT_KERNELS": ks} if ks else {}))
        written[ks] = crt_write(p, 9, n)
        assert written[ks]["text"].endswith(":generic" if ks == "generic" else ":radix8"), (ks, written[ks]["text"])
    for src, dst in itertools.permutations(cc.KERNEL_SETS, 2):
        set_switches(monkeypatch, **({"MI355_CRT_KERNELS": dst} if dst else {}))
        with CrtEngine(p, 9, n, reg_count=3) as e:
            same = (src == "generic") == (dst == "generic")
            crt_loads(e, written[src], p, image=same)
            if not same:
                e.set_int(1, SENTINEL)
                assert not e.set_data(1, written[src]["image"]) and e.get_int(1) == SENTINEL


# ---- the checkpoint file of the drivers -----------------------------------------------------------------------------------------

def test_a_checkpoint_file_of_another_plan_is_no_checkpoint(tmp_path, monkeypatch):
    """prp.save_checkpoint writes no plan; the engine's tag does.  M9941 interrupted under m2=16,c=4 and resumed on the default plan:
    load_checkpoint returns None, the run starts over from iteration 0 and ends on the right residue; resumed on its own plan it goes on"""
    set_switches(monkeypatch)
    from prmers_amd import Engine, prp
    path = str(tmp_path / "m_9941.ckpt")
    polls = [0]

    def stop():
        polls[0] += 1
        return polls[0] > 30
    with Engine(Q, prp.REGISTERS, plan="m2=16,c=4") as e:
        assert e.describe() == "marin-hip:n=512:m1=16:m2=16:c=4"
        r = prp.run_prp_or_ll(e, Q, "prp", checklevel=1, ckpt_path=path, should_stop=stop)
        assert r["interrupted"] and 0 < r["iterations"] < Q
        at = r["iterations"]
    with Engine(Q, prp.REGISTERS) as e:
        assert e.describe() == "marin-hip:n=512:m1=8:m2=32:c=4"
        assert prp.load_checkpoint(path, e, Q, "prp") is None
        msgs = []
        r = prp.run_prp_or_ll(e, Q, "prp", checklevel=1, ckpt_path=path, log=msgs.append)   # (no cadence given: it writes no checkpoint)
        assert not any("Resuming" in m for m in msgs)
        assert r["complete"] and r["is_prime"] and r["iterations"] == Q and r["gerbicz_errors"] == 0
        assert r["gerbicz_checks"] == (Q - 1) // 99 + 1                      # every boundary from iteration 0 on: nothing was resumed
    with Engine(Q, prp.REGISTERS, plan="m2=16,c=4") as e:
        got = prp.load_checkpoint(path, e, Q, "prp")
        assert got is not None and got[0] == at
        assert e.get_int(0) == pow(3, 1 << at, (1 << Q) - 1)
