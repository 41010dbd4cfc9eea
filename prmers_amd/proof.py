"""PRP proofs (GIMPS proof file, version 2) built and verified on the engine's register machine.

A PRP run saves the residue at 2^power iterations (ProofPoints: the reference's src/core/ProofSetMarin.cpp:56-122, the same
<p>/proof/<iteration> files with a CRC-32 prefix as include/mi355/caller_formats.h writes them, so either driver can finish a run
the other began).  build_proof folds them into `power` middle residues, level by level, with the hash chain deciding the
exponents (ProofSetMarin::computeProof, src/core/ProofSetMarin.cpp:213-311); the reference does every fold "A <- A^h * B" on the
host with GMP, here it is one engine call (exp_mul) on residues that never leave the device between folds.  verify_proof checks
a proof file with `power` folds and ceil(p / 2^power) squarings instead of p.

The engine is used through six methods only -- set_words, get_words, exp_mul, exp_mul2, square_mul_n, equal -- so the same code
runs on prmers_amd.Engine / CrtEngine and, in the CPU tests, on a stand-in backed by Python integers.

    python -m prmers_amd.proof build P POWER [--dir DIR] [--out FILE] [--plan SPEC] [--device N]
    python -m prmers_amd.proof verify FILE [--plan SPEC] [--device N]          (exit code 0: valid, 1: invalid)
"""
import hashlib
import os
import struct
import sys
import zlib

import numpy as np

VERIFY_REGISTERS = 5


def word_count(p):
    return (p + 31) // 32


def residue_size(p):
    """bytes of one residue in a proof file and under the hash: (p - 1) / 8 + 1"""
    return (p - 1) // 8 + 1


def _words(w, p):
    w = np.ascontiguousarray(w, dtype="<u4")
    if w.size != word_count(p):
        raise ValueError("a residue of exponent %d has %d words, not %d" % (p, word_count(p), w.size))
    return w


def residue_bytes(words, p):
    return _words(words, p).tobytes()[:residue_size(p)]


def words_from_bytes(raw, p):
    if len(raw) != residue_size(p):
        raise ValueError("a residue of exponent %d has %d bytes, not %d" % (p, residue_size(p), len(raw)))
    return np.frombuffer(raw + b"\0" * (word_count(p) * 4 - len(raw)), dtype="<u4").copy()


def res64(words):
    return (int(words[1]) << 32 if len(words) > 1 else 0) | int(words[0])


# ---------------------------------------------------------------------------------------------
# proof points
# ---------------------------------------------------------------------------------------------
def proof_points(p, power):
    """the 2^power iterations whose residues a proof of that power needs, ascending; the last one is p itself"""
    pts = [0]
    span = (p + 1) // 2
    for _ in range(power):
        pts += [x + span for x in pts]
        span = (span + 1) // 2
    pts[0] = p
    return sorted(pts)


class ProofPoints:
    """Python mirror of mi355::formats::ProofPoints: <base_dir>/<p>/proof/<iteration> = u32 CRC-32 of the words, then the words"""

    def __init__(self, p, power, base_dir="."):
        self.p, self.power = p, power
        self.dir = os.path.join(base_dir, str(p), "proof")
        self.points = proof_points(p, power)
        self._set = set(self.points)

    def should_checkpoint(self, iteration):
        return iteration in self._set

    def file_of(self, iteration):
        return os.path.join(self.dir, str(iteration))

    def save(self, iteration, words):
        if not self.should_checkpoint(iteration):
            return False
        raw = _words(words, self.p).tobytes()
        os.makedirs(self.dir, exist_ok=True)
        with open(self.file_of(iteration), "wb") as f:
            f.write(struct.pack("<I", zlib.crc32(raw) & 0xFFFFFFFF) + raw)
        return True

    def load(self, iteration):
        name = self.file_of(iteration)
        try:
            raw = open(name, "rb").read()
        except OSError:
            raise FileNotFoundError("cannot open proof checkpoint %s" % name) from None
        n = word_count(self.p) * 4
        if len(raw) < 4 + n or struct.unpack("<I", raw[:4])[0] != (zlib.crc32(raw[4:4 + n]) & 0xFFFFFFFF):
            raise ValueError("damaged proof checkpoint %s" % name)
        return np.frombuffer(raw[4:4 + n], dtype="<u4").copy()

    def valid_to(self, limit):
        return all(os.path.exists(self.file_of(pt)) for pt in self.points if pt <= limit and pt < self.p)


# ---------------------------------------------------------------------------------------------
# hash chain: SHA3-256 over the residue bytes, later levels prefixed by the previous digest; h = its first 8 bytes, little-endian
# ---------------------------------------------------------------------------------------------
def hash_residue(words, p, prefix=b""):
    return hashlib.sha3_256(prefix + residue_bytes(words, p)).digest()


def hash_chain(p, B, middles):
    """the 64-bit exponents h_0 .. h_(k-1) of a proof (B, middles)"""
    digest = hash_residue(B, p)
    hs = []
    for m in middles:
        digest = hash_residue(m, p, digest)
        hs.append(int.from_bytes(digest[:8], "little"))
    return hs


# ---------------------------------------------------------------------------------------------
# the proof and its file (ProofMarin::save / load, src/core/ProofMarin.cpp:33-199)
# ---------------------------------------------------------------------------------------------
class Proof:
    def __init__(self, p, B, middles):
        self.p = p
        self.B = _words(B, p).copy()
        self.middles = [_words(m, p).copy() for m in middles]

    @property
    def power(self):
        return len(self.middles)

    def to_bytes(self):
        head = "PRP PROOF\nVERSION=2\nHASHSIZE=64\nPOWER=%d\nNUMBER=M%d\n" % (self.power, self.p)
        return head.encode() + b"".join(residue_bytes(r, self.p) for r in [self.B] + self.middles)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @staticmethod
    def from_bytes(raw, name="proof"):
        lines, pos = [], 0
        for _ in range(5):
            e = raw.find(b"\n", pos)
            if e < 0:
                raise ValueError("%s: incomplete proof header" % name)
            lines.append(raw[pos:e].decode("ascii", "replace"))
            pos = e + 1
        if lines[0] != "PRP PROOF":
            raise ValueError("%s: not a PRP proof file" % name)
        fields = {}
        for want, line in zip(("VERSION", "HASHSIZE", "POWER", "NUMBER"), lines[1:]):
            key, eq, value = line.partition("=")
            if key != want or not eq:
                raise ValueError("%s: unexpected header line %r" % (name, line))
            fields[key] = value
        if fields["VERSION"] != "2":
            raise ValueError("%s: unsupported proof version %s" % (name, fields["VERSION"]))
        if fields["HASHSIZE"] != "64":
            raise ValueError("%s: unsupported hash size %s" % (name, fields["HASHSIZE"]))
        if not fields["POWER"].isdigit() or not 1 <= int(fields["POWER"]) <= 12:
            raise ValueError("%s: proof power %s is outside 1 .. 12" % (name, fields["POWER"]))
        number = fields["NUMBER"]
        if "/" in number:
            raise ValueError("%s: proofs of cofactors (%s) are not supported" % (name, number))
        if not (number.startswith("M") and number[1:].isdigit() and int(number[1:]) > 1):
            raise ValueError("%s: NUMBER=%s is not a Mersenne number" % (name, number))
        p, power = int(number[1:]), int(fields["POWER"])
        size = residue_size(p)
        if len(raw) - pos != size * (power + 1):
            raise ValueError("%s: %d residue bytes where power %d needs %d" % (name, len(raw) - pos, power, size * (power + 1)))
        res = [words_from_bytes(raw[pos + i * size:pos + (i + 1) * size], p) for i in range(power + 1)]
        return Proof(p, res[0], res[1:])

    @staticmethod
    def load(path):
        with open(path, "rb") as f:
            return Proof.from_bytes(f.read(), path)


def proof_file_name(p, power, directory="."):
    """<p>-<power>.proof, the reference's name (src/core/ProofManagerMarin.cpp:129-132)"""
    return os.path.join(directory, "%d-%d.proof" % (p, power))


# ---------------------------------------------------------------------------------------------
# build and verify
# ---------------------------------------------------------------------------------------------
def build_registers(power):
    """registers build_proof needs: a stack of `power` residues and one temporary"""
    return power + 1


def build_proof(engine, p, power, directory=".", log=None):
    """The proof of M_p of the given power from the point files under <directory>/<p>/proof/.

    Level L (0 .. power - 1) loads the residues at points[s (2 i + 1) - 1], s = 2^(power - L - 1), i < 2^L, pushes each on a stack
    of registers and, for every trailing one bit k of i, folds the two on top: below <- below^h * top with h = hashes[L - 1 - k]
    (exp_mul); what is left is the middle of the level, read back once (get_words), and its hash extends the chain.
    `engine` needs build_registers(power) = power + 1 registers: the stack is never deeper than `power` (level L reaches L + 1),
    register `power` is the temporary of exp_mul.  A missing or damaged point file raises an error that names it.
    log(msg) receives one line per level: "proof [L] : M <res64>, h <hash>" as the reference prints it."""
    if not 1 <= power <= 12:
        raise ValueError("proof power %d is outside 1 .. 12" % power)
    pts = ProofPoints(p, power, directory)
    tmp = power
    B = pts.load(p)
    digest = hash_residue(B, p)
    hashes, middles = [], []
    for level in range(power):
        s = 1 << (power - level - 1)
        top = 0
        for i in range(1 << level):
            engine.set_words(top, pts.load(pts.points[s * (2 * i + 1) - 1]))
            top += 1
            k = 0
            while i & (1 << k):
                top -= 1
                engine.exp_mul(top - 1, hashes[level - 1 - k], top, tmp)
                k += 1
        assert top == 1
        m = np.asarray(engine.get_words(0), dtype="<u4")
        middles.append(m)
        digest = hash_residue(m, p, digest)
        hashes.append(int.from_bytes(digest[:8], "little"))
        if log:
            log("proof [%d] : M %016x, h %016x" % (level, res64(m), hashes[-1]))
    return Proof(p, B, middles)


def verify_proof(engine, proof):
    """True when the proof shows B = 3^(2^p) mod 2^p - 1.  A = 3, B = proof.B, span = p; every middle M with its hash h halves the
    claim A^(2^span) = B:  B <- M^h * (B^2 if span is odd else B),  A <- A^h * M,  span <- (span + 1) / 2;  what is left is checked
    by `span` squarings and a comparison on the engine.  Needs VERIFY_REGISTERS = 5 registers."""
    p = proof.p
    RA, RB, RM, RM2, RT = range(VERIFY_REGISTERS)
    three = np.zeros(word_count(p), dtype="<u4")
    three[0] = 3
    engine.set_words(RA, three)
    engine.set_words(RB, proof.B)
    span = p
    for m, h in zip(proof.middles, hash_chain(p, proof.B, proof.middles)):
        engine.set_words(RM, m)
        engine.set_words(RM2, m)
        (engine.exp_mul2 if span & 1 else engine.exp_mul)(RM, h, RB, RT)   # the new B, in RM
        engine.exp_mul(RA, h, RM2, RT)
        RB, RM = RM, RB
        span = (span + 1) // 2
    engine.square_mul_n(RA, span)
    return bool(engine.equal(RA, RB))


# ---------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------
def _engine(p, registers, plan, device):
    from .engine import CrtEngine, Engine
    if plan and plan.startswith("crt"):
        parts = plan.split(":")
        odd = int(parts[1]) if len(parts) > 1 and parts[1].isdigit() else None
        return CrtEngine(p, odd, device=device, reg_count=registers)
    return Engine(p, registers, device, plan=plan)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m prmers_amd.proof", description="build or verify a PRP proof on the MI355X engine")
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build", help="fold the point files <dir>/<p>/proof/* into <p>-<power>.proof")
    b.add_argument("p", type=int)
    b.add_argument("power", type=int)
    b.add_argument("--dir", default=".")
    b.add_argument("--out", default=None)
    v = sub.add_parser("verify", help="exit code 0: the proof is valid, 1: it is not")
    v.add_argument("file")
    for x in (b, v):
        x.add_argument("--plan", default=None, help='fft_spec of the engine ("crt:9", "m2=..,c=..")')
        x.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.cmd == "build":
        with _engine(a.p, build_registers(a.power), a.plan, a.device) as e:
            proof = build_proof(e, a.p, a.power, a.dir, log=print)
        out = a.out or proof_file_name(a.p, a.power)
        proof.save(out)
        print("proof written to %s" % out)
        return 0
    proof = Proof.load(a.file)
    with _engine(proof.p, VERIFY_REGISTERS, a.plan, a.device) as e:
        ok = verify_proof(e, proof)
    print("proof of M%d, power %d: %s" % (proof.p, proof.power, "valid" if ok else "INVALID"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
