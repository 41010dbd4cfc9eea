"""PRP proofs (prmers_amd/proof.py, include/mi355/caller_formats.h) without a GPU: build and verify on a stand-in engine backed by Python
integers, every middle against a straight-line computation from the definition, rejection of tampered proofs, the exact bytes of a
proof file, and the C++ twin (its own SHA3-256 against hashlib, its proof file against the Python one)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from prmers_amd import proof as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class IntEngine:
    """the six methods proof.py uses, on Python integers mod 2^p - 1; consumed registers are poisoned"""

    def __init__(self, p, reg_count):
        self.p, self.M = p, (1 << p) - 1
        self.r = [0] * reg_count

    def set_words(self, reg, words):
        v = int.from_bytes(np.ascontiguousarray(words, dtype="<u4").tobytes(), "little")
        assert v < (1 << self.p)
        self.r[reg] = v

    def get_words(self, reg):
        v = self.r[reg] % self.M
        return np.frombuffer(v.to_bytes(P.word_count(self.p) * 4, "little"), dtype="<u4").copy()

    def _exp_mul(self, a, h, b, tmp, square):
        assert len({a, b, tmp}) == 3 and 0 <= h < 1 << 64
        y = self.r[b] * self.r[b] if square else self.r[b]
        self.r[a] = pow(self.r[a], h, self.M) * y % self.M if h else y % self.M
        self.r[b] = self.r[tmp] = None

    def exp_mul(self, a, h, b, tmp):
        self._exp_mul(a, h, b, tmp, False)

    def exp_mul2(self, a, h, b, tmp):
        self._exp_mul(a, h, b, tmp, True)

    def square_mul_n(self, reg, count, a=1, sub=0):
        assert a == 1 and sub == 0
        self.r[reg] = pow(self.r[reg], 1 << count, self.M)

    def equal(self, a, b):
        return self.r[a] % self.M == self.r[b] % self.M


def to_words(v, p):
    return np.frombuffer(int(v).to_bytes(P.word_count(p) * 4, "little"), dtype="<u4").copy()


def to_int(w):
    return int.from_bytes(np.ascontiguousarray(w, dtype="<u4").tobytes(), "little")


_RES = {}


def residues(p, power):
    """{iteration: 3^(2^iteration) mod 2^p - 1} at the proof points, by squaring from 3 (computed once per exponent)"""
    if p not in _RES:
        M = (1 << p) - 1
        want = set(P.proof_points(p, 5))
        x, out = 3, {}
        for it in range(1, p + 1):
            x = x * x % M
            if it in want:
                out[it] = x
        _RES[p] = out
    return {it: _RES[p][it] for it in P.proof_points(p, power)}


def write_points(p, power, directory):
    pts = P.ProofPoints(p, power, str(directory))
    for it, v in residues(p, power).items():
        assert pts.save(it, to_words(v, p))
    return pts


def model_proof(p, power):
    """(B, middles, hashes) as integers, straight from the definition: the middle of level L is the product over i < 2^L of
    R[points[s (2 i + 1) - 1]] ^ (product of the hashes[L - 1 - k] over the ZERO bits k < L of i), s = 2^(power - L - 1)"""
    M = (1 << p) - 1
    res = residues(p, power)
    pts = sorted(res)
    nbytes = (p - 1) // 8 + 1
    B = res[p]
    digest = hashlib.sha3_256(B.to_bytes(nbytes, "little")).digest()
    hashes, middles = [], []
    for L in range(power):
        s = 1 << (power - L - 1)
        m = 1
        for i in range(1 << L):
            e = 1
            for k in range(L):
                if not (i >> k) & 1:
                    e *= hashes[L - 1 - k]
            m = m * pow(res[pts[s * (2 * i + 1) - 1]], e, M) % M
        middles.append(m)
        digest = hashlib.sha3_256(digest + m.to_bytes(nbytes, "little")).digest()
        hashes.append(int.from_bytes(digest[:8], "little"))
    return B, middles, hashes


CASES = [(p, k) for p in (127, 521, 9941) for k in (1, 2, 3, 5)]


def test_points_match_the_closed_form_and_the_cpp_rule():
    """2^power points, the last one p, each a sum of a subset of the spans (p+1)/2, ceil of that / 2, ...: ProofSetMarin.cpp:64-92"""
    for p, k in CASES + [(11213, 3), (136279841, 8)]:
        pts = P.proof_points(p, k)
        assert len(pts) == 1 << k == len(set(pts)) and pts == sorted(pts) and pts[-1] == p and pts[0] >= 1
        spans, s = [], (p + 1) // 2
        for _ in range(k):
            spans.append(s)
            s = (s + 1) // 2
        sums = {sum(sp for j, sp in enumerate(spans) if (mask >> j) & 1) for mask in range(1, 1 << k)} | {p}
        assert set(pts) == sums
    assert P.proof_points(127, 2) == [32, 64, 96, 127]


@pytest.mark.parametrize("p,power", CASES)
def test_build_and_verify_on_the_integer_engine(p, power, tmp_path):
    write_points(p, power, tmp_path)
    lines = []
    pr = P.build_proof(IntEngine(p, P.build_registers(power)), p, power, str(tmp_path), log=lines.append)
    B, middles, hashes = model_proof(p, power)
    assert to_int(pr.B) == B and pr.power == power
    for L in range(power):
        assert to_int(pr.middles[L]) == middles[L], (p, power, L)
        assert lines[L] == "proof [%d] : M %016x, h %016x" % (L, middles[L] & (2 ** 64 - 1), hashes[L])
    assert P.hash_chain(p, pr.B, pr.middles) == hashes
    assert P.verify_proof(IntEngine(p, P.VERIFY_REGISTERS), pr) is True
    # through the file
    name = P.proof_file_name(p, power, str(tmp_path))
    assert os.path.basename(name) == "%d-%d.proof" % (p, power)
    pr.save(name)
    back = P.Proof.load(name)
    assert back.p == p and np.array_equal(back.B, pr.B) and all(np.array_equal(a, b) for a, b in zip(back.middles, pr.middles))
    assert P.verify_proof(IntEngine(p, P.VERIFY_REGISTERS), back) is True


def test_verify_is_the_claim_about_b_and_not_about_the_file(tmp_path):
    """a proof built honestly from residues of a WRONG chain (start 5 instead of 3) does not verify"""
    p, power = 521, 3
    M = (1 << p) - 1
    pts = P.ProofPoints(p, power, str(tmp_path))
    x = 5
    for it in range(1, p + 1):
        x = x * x % M
        pts.save(it, to_words(x, p))
    pr = P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path))
    assert P.verify_proof(IntEngine(p, 5), pr) is False


@pytest.mark.parametrize("p,power", [(127, 2), (521, 3), (9941, 5)])
def test_tampered_proofs_are_rejected(p, power, tmp_path):
    write_points(p, power, tmp_path)
    pr = P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path))
    good = pr.to_bytes()
    head = good.index(b"NUMBER=") + len("NUMBER=M%d\n" % p)
    size = (p - 1) // 8 + 1
    assert len(good) == head + size * (power + 1)

    def verdict(raw):
        return P.verify_proof(IntEngine(p, 5), P.Proof.from_bytes(raw))

    assert verdict(good) is True
    for which in range(power + 1):                      # one flipped bit in B (0) and in every middle
        raw = bytearray(good)
        raw[head + which * size + size // 2] ^= 0x10
        assert verdict(bytes(raw)) is False, which
    # the power in the header: one less leaves a file that is too long, one more a file that is too short -- both refused by load
    for other in (power - 1, power + 1):
        raw = good.replace(b"POWER=%d\n" % power, b"POWER=%d\n" % other)
        with pytest.raises(ValueError):
            P.Proof.from_bytes(raw)
    # (cutting the last middle off as well is no tampering: the first k - 1 middles of a proof ARE the proof of power k - 1)
    if power > 1:
        raw = good.replace(b"POWER=%d\n" % power, b"POWER=%d\n" % (power - 1))[:-size]
        assert verdict(raw) is True


def test_load_rejects_what_it_does_not_support():
    p = 127
    body = bytes(16 * 3)
    ok = b"PRP PROOF\nVERSION=2\nHASHSIZE=64\nPOWER=2\nNUMBER=M127\n" + body
    assert P.Proof.from_bytes(ok).power == 2
    for bad in (ok.replace(b"VERSION=2", b"VERSION=1"), ok.replace(b"HASHSIZE=64", b"HASHSIZE=32"), ok.replace(b"POWER=2", b"POWER=0"),
                ok.replace(b"POWER=2", b"POWER=13"), ok.replace(b"NUMBER=M127", b"NUMBER=M127/2349023"), ok[:-1], ok + b"\0",
                ok.replace(b"PRP PROOF", b"PRP PROOFS"), ok.replace(b"NUMBER=M127", b"NUMBER=127"), ok[:30]):
        with pytest.raises(ValueError):
            P.Proof.from_bytes(bad)


def test_missing_or_damaged_point_file_is_named(tmp_path):
    p, power = 521, 3
    pts = write_points(p, power, tmp_path)
    victim = pts.points[2]
    os.remove(pts.file_of(victim))
    with pytest.raises(FileNotFoundError, match=pts.file_of(victim).replace("\\", "\\\\")):
        P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path))
    pts.save(victim, to_words(residues(p, power)[victim], p))
    raw = bytearray(open(pts.file_of(pts.points[4]), "rb").read())
    raw[9] ^= 1
    open(pts.file_of(pts.points[4]), "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="damaged proof checkpoint .*%d$" % pts.points[4]):
        P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path))


def test_proof_file_bytes_p127_power2(tmp_path):
    """header, then B and the two middles, 16 little-endian bytes each; the point files carry a CRC-32 in front of 4 words"""
    p, power = 127, 2
    pts = write_points(p, power, tmp_path)
    one = open(pts.file_of(32), "rb").read()
    import zlib
    assert len(one) == 4 + 16 and int.from_bytes(one[:4], "little") == zlib.crc32(one[4:]) and one[4:] == pow(3, 1 << 32, (1 << 127) - 1).to_bytes(16, "little")
    assert sorted(os.listdir(tmp_path / "127" / "proof")) == ["127", "32", "64", "96"]
    pr = P.build_proof(IntEngine(p, 3), p, power, str(tmp_path))
    B, middles, _ = model_proof(p, power)
    assert B == 9                                       # M127 is prime: 3^(2^127) = 9
    want = b"PRP PROOF\nVERSION=2\nHASHSIZE=64\nPOWER=2\nNUMBER=M127\n" + b"".join(v.to_bytes(16, "little") for v in [B] + middles)
    name = str(tmp_path / "x.proof")
    pr.save(name)
    assert open(name, "rb").read() == want == pr.to_bytes()
    assert middles[0] == pow(3, 1 << 64, (1 << 127) - 1)


def test_run_prp_saves_the_points_and_survives_a_resume(tmp_path):
    """run_prp_or_ll(proof_power=k) on the CPU oracle: the point files of a run in one piece and of a run stopped and resumed from
    a checkpoint are the residues 3^(2^i); the default (0) writes nothing"""
    import orc
    from prmers_amd import prp
    p, power = 521, 3
    d1, d2 = tmp_path / "a", tmp_path / "b"
    r = prp.run_prp_or_ll(orc.OracleEngine(p, 8), p, proof_power=power, proof_dir=str(d1))
    assert r["complete"] and r["is_prime"]
    ck = str(tmp_path / "m.ckpt")
    e = orc.OracleEngine(p, 8)
    r1 = prp.run_prp_or_ll(e, p, proof_power=power, proof_dir=str(d2), ckpt_path=ck, backup_every=100, max_iters=300)
    assert not r1["complete"]
    r2 = prp.run_prp_or_ll(orc.OracleEngine(p, 8), p, proof_power=power, proof_dir=str(d2), ckpt_path=ck)
    assert r2["complete"] and r2["res64"] == r["res64"]
    for d in (d1, d2):
        pts = P.ProofPoints(p, power, str(d))
        for it, v in residues(p, power).items():
            assert to_int(pts.load(it)) == v, (d, it)
        pr = P.build_proof(IntEngine(p, power + 1), p, power, str(d))
        assert P.verify_proof(IntEngine(p, 5), pr)
    prp.run_prp_or_ll(orc.OracleEngine(p, 8), p, proof_dir=str(tmp_path / "c"))
    assert not (tmp_path / "c").exists()


# ---- the C++ twin ------------------------------------------------------------------------------------------------------------

def _build_cpp(td):
    exe = os.path.join(str(td), "t_proof_formats")
    gmp = "/usr/lib/x86_64-linux-gnu/libgmp.so.10"
    inc = [i for i in ("/opt/conda/include", "/usr/include") if os.path.exists(os.path.join(i, "gmp.h"))]
    if not inc or not os.path.exists(gmp):
        pytest.skip("gmp headers/library not available")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + inc[0], "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_proof_formats.cpp"), gmp])
    return exe


def test_cpp_sha3_and_proof_file_match_python(tmp_path):
    exe = _build_cpp(tmp_path)
    # SHA3-256 of i * 7 + 1 mod 256 patterns at the lengths around the rate (136 bytes)
    for n in (0, 3, 135, 136, 137, 200):
        data = bytes((i * 7 + 1) & 0xFF for i in range(n))
        out = subprocess.run([exe, "sha3", str(n)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == hashlib.sha3_256(data).hexdigest(), (n, out.stdout, out.stderr)
    # points written by Python, proof built by the C++ code on a GMP stand-in engine: the same file, and its verifier accepts it
    p, power = 9941, 3
    write_points(p, power, tmp_path)
    pr = P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path))
    py_name, cpp_name = str(tmp_path / "py.proof"), str(tmp_path / "cpp.proof")
    pr.save(py_name)
    out = subprocess.run([exe, "build", str(p), str(power), str(tmp_path), cpp_name], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(cpp_name, "rb").read() == open(py_name, "rb").read()
    B, middles, hashes = model_proof(p, power)
    assert [l for l in out.stdout.splitlines() if l.startswith("proof [")] == \
        ["proof [%d] : M %016x, h %016x" % (L, middles[L] & (2 ** 64 - 1), hashes[L]) for L in range(power)]
    assert subprocess.run([exe, "verify", py_name]).returncode == 0
    raw = bytearray(open(py_name, "rb").read())
    raw[-700] ^= 4
    bad = str(tmp_path / "bad.proof")
    open(bad, "wb").write(bytes(raw))
    assert subprocess.run([exe, "verify", bad]).returncode == 1
    # points written by the C++ ProofPoints are the files Python reads
    out = subprocess.run([exe, "points", str(p), str(power), str(tmp_path / "cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [int(x) for x in out.stdout.split()] == P.proof_points(p, power)
    a, b = P.ProofPoints(p, power, str(tmp_path / "cpp")), P.ProofPoints(p, power, str(tmp_path))
    for it in a.points:
        assert open(a.file_of(it), "rb").read() == open(b.file_of(it), "rb").read()


def test_cpp_driver_builds_and_verifies_a_proof_on_the_oracle(tmp_path):
    """examples/prp_cli.cpp -proof / -verify on CPU: engine_hip loading the oracle-backed ABI shim, which has neither the word entry
    points nor exp_mul, so the adapter's compositions run.  The file is the one the Python code builds on integers."""
    exe = os.path.join(str(tmp_path), "mi355_prp")
    gmp = "/usr/lib/x86_64-linux-gnu/libgmp.so.10"
    inc = [i for i in ("/opt/conda/include", "/usr/include") if os.path.exists(os.path.join(i, "gmp.h"))]
    if not inc or not os.path.exists(gmp):
        pytest.skip("gmp headers/library not available")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + inc[0], "-o", exe,
                           os.path.join(ROOT, "examples", "prp_cli.cpp"), "-ldl", gmp])
    shim = os.path.join(str(tmp_path), "liboracle_abi_shim.so")
    subprocess.check_call(["gcc", "-O3", "-fopenmp", "-fPIC", "-shared", "-fvisibility=hidden", "-o", shim,
                           os.path.join(ROOT, "tests", "host", "oracle_abi_shim.c"), os.path.join(ROOT, "oracle", "oracle.c"), "-lm"])
    env = dict(os.environ, OMP_NUM_THREADS="2")
    p, power = 521, 2
    o = subprocess.run([exe, str(p), "-proof", str(power), "-lib", shim], capture_output=True, text=True, cwd=str(tmp_path), env=env)
    assert o.returncode == 0 and "probably prime" in o.stdout and "Proof file: 521-2.proof" in o.stdout, o.stdout + o.stderr
    write_points(p, power, tmp_path / "py")
    want = P.build_proof(IntEngine(p, power + 1), p, power, str(tmp_path / "py"))
    got = (tmp_path / "521-2.proof").read_bytes()
    assert got == want.to_bytes()
    _, middles, hashes = model_proof(p, power)
    assert [l for l in o.stdout.splitlines() if l.startswith("proof [")] == \
        ["proof [%d] : M %016x, h %016x" % (L, middles[L] & (2 ** 64 - 1), hashes[L]) for L in range(power)]
    v = subprocess.run([exe, "-verify", "521-2.proof", "-lib", shim], capture_output=True, text=True, cwd=str(tmp_path), env=env)
    assert v.returncode == 0 and "valid" in v.stdout, v.stdout + v.stderr
    bad = bytearray(got)
    bad[-20] ^= 1
    (tmp_path / "bad.proof").write_bytes(bytes(bad))
    v = subprocess.run([exe, "-verify", "bad.proof", "-lib", shim], capture_output=True, text=True, cwd=str(tmp_path), env=env)
    assert v.returncode == 1 and "INVALID" in v.stdout, v.stdout + v.stderr
