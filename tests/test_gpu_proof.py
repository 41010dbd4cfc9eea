"""exp_mul / exp_mul2 of both engines against integers, and PRP proofs end to end on the MI355X: the points of a real run (resumed from a
checkpoint once), build_proof and verify_proof on the engine, the same file as the integer stand-in of tests/test_proof.py produces, the
second field family, and the C++ driver.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import os
import subprocess

import numpy as np
import pytest

from prmers_amd import proof as P
from test_proof import IntEngine, model_proof, to_int, to_words, write_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_engine(p, family, regs):
    from prmers_amd import CrtEngine, Engine
    # (the radix-9 axis needs more than 15 bits per word: p = 127 takes the plain power-of-two size of this family, n = 8)
    return CrtEngine(p, 9 if p > 1000 else 1, reg_count=regs) if family == "crt" else Engine(p, regs)


@pytest.mark.parametrize("family", ["goldilocks", "crt"])
@pytest.mark.parametrize("p", [127, 9941])
def test_exp_mul_against_integers(p, family):
    from prmers_amd import EngineError
    rng = np.random.default_rng(p)
    Mp = (1 << p) - 1
    hs = [0, 1, 2, 1 << 63, (1 << 64) - 1] + [int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) for _ in range(3)]
    rnd = lambda: int.from_bytes(rng.bytes((p + 7) // 8), "little") % Mp   # noqa: E731
    with make_engine(p, family, 4) as e:
        for h in hs:
            for name, sq in (("exp_mul", 1), ("exp_mul2", 2)):
                a, b = rnd(), rnd()
                e.set_int(0, a); e.set_int(2, b); e.set_int(1, 12345)
                getattr(e, name)(0, h, 2, 1)
                want = pow(a, h, Mp) * pow(b, sq, Mp) % Mp if h else pow(b, sq, Mp)
                assert e.get_int(0) == want, (p, family, name, hex(h))
        # b and tmp are consumed: they hold multiplicand images now, which is no residue
        for consumed in (1, 2):
            with pytest.raises(EngineError, match="image"):
                e.words(consumed)
        # refused: aliased registers, a register out of range, an operand that holds an image; the result register is untouched
        e.set_int(0, 77); e.set_int(3, 5)
        for args in ((0, 3, 0, 1), (0, 3, 3, 0), (0, 3, 3, 3), (3, 3, 3, 0), (0, 3, 3, 9), (9, 3, 3, 1), (0, 3, 2, 3), (2, 3, 0, 3)):
            for name in ("exp_mul", "exp_mul2"):
                with pytest.raises(EngineError):
                    getattr(e, name)(*args)
        with pytest.raises(ValueError):
            e.exp_mul(0, 1 << 64, 3, 1)
        with pytest.raises(ValueError):
            e.exp_mul(0, -1, 3, 1)
        assert e.get_int(0) == 77 and e.get_int(3) == 5
        # ... and the engine still works
        e.exp_mul(0, 3, 3, 1)
        assert e.get_int(0) == 77 ** 3 * 5 % Mp


def run_with_points(p, family, power, directory, resume):
    """a PRP run of M_p that leaves its proof points under `directory`; resume: in two pieces, the second from the checkpoint of the first"""
    from prmers_amd import prp
    ck = os.path.join(directory, "m.ckpt")
    if resume:
        with make_engine(p, family, prp.REGISTERS) as e:
            r = prp.run_prp_or_ll(e, p, proof_power=power, proof_dir=directory, ckpt_path=ck, backup_every=1000, max_iters=p // 2 + 37)
            assert not r["complete"]
    with make_engine(p, family, prp.REGISTERS) as e:
        r = prp.run_prp_or_ll(e, p, proof_power=power, proof_dir=directory, ckpt_path=ck if resume else None)
    assert r["complete"] and r["is_prime"] and r["gerbicz_errors"] == 0
    return r


@pytest.mark.parametrize("p,family,resume", [(9941, "goldilocks", True), (11213, "goldilocks", False), (9941, "crt", False)])
def test_proof_end_to_end(p, family, resume, tmp_path):
    power = 3
    run_with_points(p, family, power, str(tmp_path), resume)
    B, middles, hashes = model_proof(p, power)
    pts = P.ProofPoints(p, power, str(tmp_path))
    assert pts.valid_to(p) and to_int(pts.load(p)) == B == 9
    lines = []
    with make_engine(p, family, P.build_registers(power)) as e:
        pr = P.build_proof(e, p, power, str(tmp_path), log=lines.append)
    assert to_int(pr.B) == B and [to_int(m) for m in pr.middles] == middles
    assert lines == ["proof [%d] : M %016x, h %016x" % (L, middles[L] & (2 ** 64 - 1), hashes[L]) for L in range(power)]
    # the same bytes as the integer stand-in makes from points written by the test
    write_points(p, power, tmp_path / "model")
    want = P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path / "model")).to_bytes()
    name = P.proof_file_name(p, power, str(tmp_path))
    pr.save(name)
    assert open(name, "rb").read() == want
    with make_engine(p, family, P.VERIFY_REGISTERS) as e:
        assert P.verify_proof(e, P.Proof.load(name)) is True
        # one flipped bit, in a middle and in B
        for at in (len(want) - 40, len(want) - (power + 1) * ((p - 1) // 8 + 1) + 3):
            bad = bytearray(want)
            bad[at] ^= 0x20
            assert P.verify_proof(e, P.Proof.from_bytes(bytes(bad))) is False
        assert P.verify_proof(e, pr) is True


def test_proof_command_line(tmp_path):
    """python -m prmers_amd.proof build | verify, in processes of their own"""
    import sys
    p, power = 9941, 2
    write_points(p, power, tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *a: subprocess.run([sys.executable, "-m", "prmers_amd.proof", *a], capture_output=True, text=True, cwd=str(tmp_path), env=env)   # noqa: E731
    o = run("build", str(p), str(power))
    assert o.returncode == 0 and "proof [1]" in o.stdout, o.stdout + o.stderr
    want = P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path)).to_bytes()
    assert (tmp_path / "9941-2.proof").read_bytes() == want
    assert run("verify", "9941-2.proof").returncode == 0
    assert run("verify", "9941-2.proof", "--plan", "crt:9").returncode == 0
    bad = bytearray(want)
    bad[-5] ^= 1
    (tmp_path / "bad.proof").write_bytes(bytes(bad))
    o = run("verify", "bad.proof")
    assert o.returncode == 1 and "INVALID" in o.stdout, o.stdout + o.stderr


def test_cpp_driver_proof_and_verify(tmp_path):
    """examples/prp_cli.cpp: -proof 2 on M9941 writes 9941-2.proof, -verify accepts it and refuses a copy with a flipped byte; the Python
    verifier accepts the C++ file"""
    from prmers_amd import Engine, engine as E
    exe = os.path.join(str(tmp_path), "mi355_prp")
    gmp = "/usr/lib/x86_64-linux-gnu/libgmp.so.10"
    inc = [i for i in ("/opt/conda/include", "/usr/include") if os.path.exists(os.path.join(i, "gmp.h"))]
    if not inc or not os.path.exists(gmp):
        pytest.skip("gmp headers/library not available")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + inc[0], "-o", exe,
                           os.path.join(ROOT, "examples", "prp_cli.cpp"), "-ldl", gmp])
    run = lambda *a: subprocess.run([exe, *a, "-lib", E.LIB_PATH], capture_output=True, text=True, cwd=str(tmp_path))   # noqa: E731
    p, power = 9941, 2
    o = run(str(p), "-proof", str(power))
    assert o.returncode == 0 and "probably prime" in o.stdout and "Proof file: 9941-2.proof" in o.stdout, o.stdout + o.stderr
    _, middles, hashes = model_proof(p, power)
    assert [l for l in o.stdout.splitlines() if l.startswith("proof [")] == \
        ["proof [%d] : M %016x, h %016x" % (L, middles[L] & (2 ** 64 - 1), hashes[L]) for L in range(power)]
    got = (tmp_path / "9941-2.proof").read_bytes()
    write_points(p, power, tmp_path / "model")
    assert got == P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path / "model")).to_bytes()
    # the C++ run's point files are the ones Python reads
    assert to_int(P.ProofPoints(p, power, str(tmp_path)).load(p)) == 9
    v = run("-verify", "9941-2.proof")
    assert v.returncode == 0 and "valid" in v.stdout, v.stdout + v.stderr
    assert run("-verify", "9941-2.proof", "-fft", "crt:9").returncode == 0
    bad = bytearray(got)
    bad[len(bad) // 2] ^= 0x40
    (tmp_path / "bad.proof").write_bytes(bytes(bad))
    v = run("-verify", "bad.proof")
    assert v.returncode == 1 and "INVALID" in v.stdout, v.stdout + v.stderr
    with Engine(p, P.VERIFY_REGISTERS) as e:
        assert P.verify_proof(e, P.Proof.load(str(tmp_path / "9941-2.proof"))) is True
