"""The two files of an ECM run that outlive its process (prmers_amd/ecm.py writes and reads them; no engine in here).

Resume lines:  the stage-1 result of one curve as GMP-ECM and Prime95 exchange it (the reference: its -resume / -p95 output), one line a curve:

    METHOD=ECM; SIGMA=824476324263488495; B1=20000; N=2^149-1; X=0x1dbf...; CHECKSUM=1732255967; PROGRAM=...; X0=0x0; Y0=0x0; TIME=...;

          SIGMA is Suyama's parameter (ecm.suyama; GMP-ECM's PARAM=0), X the affine x = X_Q / Z_Q of Q = E(B1) P on the Montgomery curve of
          that sigma, and CHECKSUM = B1 (SIGMA mod M) (N mod M) (X mod M) mod M with M = 4294967291, the largest prime below 2^32.  A line
          exists only for a curve whose Z_Q is invertible modulo N.  N is always a Mersenne number here.
Checkpoints:   the state of an interrupted stage 1 of one group of curves (one curve, or one curve a lane), in one file: a JSON header on the
          first line, then a binary payload.  The header holds the format version, p, b1, b2, D, the curve form, the sigmas as drawn and the
          lanes that ride on a substitute curve, the bit length and SHA-256 of the stage-1 scalar, the index of the next scalar digit,
          the group index of ecm.ecm(), the shape of the payload and its SHA-256.  The payload holds the CANONICAL residues of the point
          registers, lanes x word_count little-endian 32-bit words a register -- what Engine.words_lanes returns -- so a checkpoint does
          not depend on the transform plan, on onelaunch, on batches or on the kernel set, and a run continued from it reaches the same
          residues: the arithmetic is exact modulo 2^p - 1.  The file is written under a temporary name in the same directory and moved
          into place with os.replace, so a reader sees the old file or the new one, never a part.
"""
import hashlib
import json
import os
import time as _time

CHECKSUM_MODULUS = 4294967291
CHECKPOINT_VERSION = 1
PROGRAM = "prmers_amd"


class ResumeFormatError(ValueError):
    """a resume line that cannot be used; the message says why"""


class CheckpointError(RuntimeError):
    """a checkpoint file that cannot be read, or that belongs to another run; the message says why"""


# ---- resume lines -------------------------------------------------------------------------------------------------------------------------

def checksum(b1, sigma, n, x):
    """B1 (sigma mod M) (n mod M) (x mod M) mod M, M = 4294967291"""
    M = CHECKSUM_MODULUS
    return int(b1) * (int(sigma) % M) % M * (int(n) % M) % M * (int(x) % M) % M


def resume_line(p, sigma, b1, x, program=PROGRAM, time=None):
    """the line of the curve `sigma` on 2^p - 1 after a stage 1 to b1 that ended in the affine x; time: the text of TIME (None: now)"""
    n = (1 << p) - 1
    if not 0 <= x < n:
        raise ValueError("x must be a residue modulo 2^%d - 1" % p)
    if time is None:
        time = _time.strftime("%a %b %d %H:%M:%S %Y")
    return "METHOD=ECM; SIGMA=%d; B1=%d; N=2^%d-1; X=0x%x; CHECKSUM=%d; PROGRAM=%s; X0=0x0; Y0=0x0; TIME=%s;" % (
        sigma, b1, p, x, checksum(b1, sigma, n, x), program, time)


def _integer(name, text):
    """a decimal or 0x integer"""
    try:
        return int(text, 16) if text.lower().startswith("0x") else int(text)
    except ValueError:
        raise ResumeFormatError("%s=%s is not a decimal or 0x integer" % (name, text[:40])) from None


def _bound(text):
    """B1: an integer, also where it is written the way a floating-point number is (2e4, 20000.0)"""
    try:
        return int(text)
    except ValueError:
        pass
    try:
        v = float(text)
    except ValueError:
        v = None
    if v is None or v != int(v):
        raise ResumeFormatError("B1=%s is not an integer" % text[:40])
    return int(v)


def _mersenne_exponent(text):
    """p of N = 2^p - 1, from `2^p-1` or from a decimal or 0x integer of that value"""
    t = text.replace(" ", "")
    if t.startswith("2^") and t.endswith("-1") and t[2:-2].isdigit():
        p = int(t[2:-2])
    else:
        n = _integer("N", t)
        p = n.bit_length()
        if n < 3 or n & (n + 1):
            raise ResumeFormatError("N is no 2^p - 1 (a number of %d bits): this project factors Mersenne numbers" % p)
    if p < 2:
        raise ResumeFormatError("N = 2^%d - 1 has no exponent to speak of" % p)
    return p


def parse_resume_line(line):
    """-> {"p", "sigma", "b1", "x"} of a resume line.  Fields come in any order and unknown ones are ignored; N is 2^p-1 or an integer of
    that value; X and SIGMA are decimal or 0x; PARAM=0 is accepted.  ResumeFormatError for a method other than ECM, a PARAM other than 0,
    an N that is no 2^p - 1, x >= N, a missing field and a CHECKSUM that is present and wrong."""
    fields = {}
    for part in line.strip().split(";"):
        if "=" in part:
            k, v = part.split("=", 1)
            fields.setdefault(k.strip().upper(), v.strip())
    method = fields.get("METHOD")
    if method is None or method.upper() != "ECM":
        raise ResumeFormatError("METHOD=%s: only ECM lines are read here" % method)
    if "PARAM" in fields and _integer("PARAM", fields["PARAM"]) != 0:
        raise ResumeFormatError("PARAM=%s: only Suyama's sigma (PARAM=0) is known here" % fields["PARAM"])
    for k in ("SIGMA", "B1", "N", "X"):
        if k not in fields:
            raise ResumeFormatError("the line has no %s" % k)
    p = _mersenne_exponent(fields["N"])
    sigma, b1, x = _integer("SIGMA", fields["SIGMA"]), _bound(fields["B1"]), _integer("X", fields["X"])
    n = (1 << p) - 1
    if sigma < 0 or b1 < 2:
        raise ResumeFormatError("SIGMA=%d, B1=%d: out of range" % (sigma, b1))
    if not 0 <= x < n:
        raise ResumeFormatError("X is not below N = 2^%d - 1" % p)
    if "CHECKSUM" in fields:
        given, want = _integer("CHECKSUM", fields["CHECKSUM"]), checksum(b1, sigma, n, x)
        if given != want:
            raise ResumeFormatError("CHECKSUM=%d, but B1, SIGMA, N and X give %d: the line is damaged" % (given, want))
    return {"p": p, "sigma": sigma, "b1": b1, "x": x}


def read_resume_file(path):
    """[parse_resume_line(line) for the lines of the file], blank lines and # lines skipped; an error names the line's number"""
    out = []
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            try:
                out.append(parse_resume_line(line))
            except ResumeFormatError as err:
                raise ResumeFormatError("%s, line %d: %s" % (path, number, err)) from None
    return out


def append_resume_lines(path, lines):
    """whole lines at the end of the file, flushed before the call returns"""
    lines = [l.rstrip("\n") for l in lines]
    if any("\n" in l for l in lines):
        raise ValueError("a resume line is one line")
    if not lines:
        return
    with open(path, "a") as f:
        f.write("".join(l + "\n" for l in lines))
        f.flush()
        os.fsync(f.fileno())


# ---- stage-1 checkpoints ------------------------------------------------------------------------------------------------------------------

def scalar_digest(e):
    """(bit length, SHA-256 of the little-endian bytes) of the stage-1 scalar: what a checkpoint says about it instead of its megabytes"""
    e = int(e)
    return e.bit_length(), hashlib.sha256(e.to_bytes((e.bit_length() + 7) // 8 or 1, "little")).hexdigest()


def word_count(p):
    return (p + 31) // 32


HEADER_KEYS = ("version", "p", "b1", "b2", "D", "curve", "sigmas", "substitutes", "scalar_bits", "scalar_sha256", "next", "group",
               "registers", "lanes", "word_count", "payload_sha256")


def write_checkpoint(path, header, registers):
    """header: p, b1, b2, D, curve, sigmas, substitutes, scalar_bits, scalar_sha256, next, group; registers: for every point register the
    canonical residues of its lanes as integers.  Version, shape and digest are added here.  The file appears under `path` whole."""
    header = dict(header)
    p = header["p"]
    wc = word_count(p)
    lanes = len(registers[0])
    if any(len(r) != lanes for r in registers) or lanes != len(header["sigmas"]):
        raise ValueError("a checkpoint holds one residue per sigma in every register")
    payload = b"".join(int(v).to_bytes(4 * wc, "little") for r in registers for v in r)
    header.update(version=CHECKPOINT_VERSION, registers=len(registers), lanes=lanes, word_count=wc,
                  payload_sha256=hashlib.sha256(payload).hexdigest())
    missing = [k for k in HEADER_KEYS if k not in header]
    if missing:
        raise ValueError("the checkpoint header lacks %s" % ", ".join(missing))
    path = os.fspath(path)
    tmp = os.path.join(os.path.dirname(path) or ".", ".%s.%d.tmp" % (os.path.basename(path), os.getpid()))
    try:
        with open(tmp, "wb") as f:
            f.write(json.dumps(header, sort_keys=True).encode("ascii") + b"\n")
            f.write(payload)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def read_checkpoint(path):
    """-> (header, registers) as write_checkpoint took them.  CheckpointError on a short file, a wrong digest or an unknown version."""
    with open(path, "rb") as f:
        raw = f.read()
    cut = raw.find(b"\n")
    if cut < 0:
        raise CheckpointError("%s: short file, the header does not end" % path)
    try:
        header = json.loads(raw[:cut].decode("ascii"))
    except ValueError:
        raise CheckpointError("%s: the header is not JSON" % path) from None
    if not isinstance(header, dict) or header.get("version") != CHECKPOINT_VERSION:
        raise CheckpointError("%s: format version %r, this code reads version %d"
                              % (path, header.get("version") if isinstance(header, dict) else None, CHECKPOINT_VERSION))
    missing = [k for k in HEADER_KEYS if k not in header]
    if missing:
        raise CheckpointError("%s: the header lacks %s" % (path, ", ".join(missing)))
    payload = raw[cut + 1:]
    regs, lanes, wc = header["registers"], header["lanes"], header["word_count"]
    if wc != word_count(header["p"]) or lanes != len(header["sigmas"]):
        raise CheckpointError("%s: the header's shape does not fit its p and sigmas" % path)
    if len(payload) != regs * lanes * wc * 4:
        raise CheckpointError("%s: %s, %d payload bytes where the header promises %d"
                              % (path, "short file" if len(payload) < regs * lanes * wc * 4 else "long file", len(payload), regs * lanes * wc * 4))
    if hashlib.sha256(payload).hexdigest() != header["payload_sha256"]:
        raise CheckpointError("%s: the payload's SHA-256 is not the header's" % path)
    size = 4 * wc
    registers = [[int.from_bytes(payload[(r * lanes + l) * size:(r * lanes + l + 1) * size], "little") for l in range(lanes)]
                 for r in range(regs)]
    return header, registers
