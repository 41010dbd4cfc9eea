#!/usr/bin/env python3
"""Generate tests/golden/reference_outputs.json: what the reference's own programs print or write for the inputs of the
tests that pin the oracles against them (tests/test_oracle_golden.py, tests/test_oracle_crt.py), recorded once so that the
suite needs neither the reference tree nor oracle/_ref.

Inputs are rebuilt exactly as the tests build them (same exponents, same seeds, digit vectors from the oracle); the outputs
are those of oracle/_ref/ref_host (the reference's host headers: transform size, IBDWT tables, digit formatting, set_mpz) and
oracle/_ref/ref_mixed_crt (the reference's CPU prototype of the paired-NTT path).  Tables and long hex strings are stored as
SHA-256 digests, and the prototype's timing figures are cut from its lines.  Needs oracle/_ref (`make -C oracle ref`, only where
the reference tree is present) and the built oracle.
Run: python tests/golden/make_reference_outputs.py
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orc  # noqa: E402

REF_HOST = os.path.join(ROOT, "oracle", "_ref", "ref_host")
REF_CRT = os.path.join(ROOT, "oracle", "_ref", "ref_mixed_crt")

TABLE_EXPONENTS = [31, 89, 127, 521, 1279, 3001, 9941, 100003, 1000003, 2500007]
DIGIT_EXPONENTS = [127, 9941, 100003]
LL_CASES = [(1279, 9), (2203, 3), (2281, 9), (2293, 9), (4253, 3), (4423, 9), (9941, 9), (9949, 3)]


def size_exponents():
    rng = np.random.default_rng(7)
    return [3, 5, 31, 61, 89, 127, 1279, 86243, 9815459, 57885161, 136279841, 205271257, 600000001, 2147483647] + \
        [int(x) for x in rng.integers(100, 2**31, 40)]


def digit_cases(p):
    """the digit vectors of test_digit_formatting_matches_reference_headers, in its order"""
    M = (1 << p) - 1
    rng = np.random.default_rng(p)
    o = orc.Oracle(p, 2)
    out = []
    for v in [9, 0, M, 3, int.from_bytes(rng.bytes((p + 7) // 8), "little") % M]:
        if v == M:
            d = o.widths().astype(np.uint64)
            d = ((np.uint64(1) << d) - np.uint64(1)) | (d << np.uint64(32))
        else:
            o.set_value(0, v)
            d = o.digits(0)
        out.append((v, d))
    return out


def sha(b):
    return hashlib.sha256(b).hexdigest()


def main():
    for exe in (REF_HOST, REF_CRT):
        if not os.path.exists(exe):
            raise SystemExit("%s missing: build it with `make -C oracle ref` where the reference tree is present" % exe)
    res = {"_source": "outputs of the reference's own host code (oracle/_ref/ref_host) and CPU prototype (oracle/_ref/ref_mixed_crt); "
                      "data only, written by tests/golden/make_reference_outputs.py"}
    res["transform_size"] = {str(p): int(subprocess.check_output([REF_HOST, "size", str(p)]).split()[0]) for p in size_exponents()}
    tables = {}
    with tempfile.TemporaryDirectory() as td:
        for p in TABLE_EXPONENTS:
            out = os.path.join(td, "t.bin")
            subprocess.check_call([REF_HOST, "tables", str(p), out])
            raw = open(out, "rb").read()
            n = int(np.frombuffer(raw[:8], dtype=np.uint64)[0])
            tables[str(p)] = {"n": n, "sha256_width_u8": sha(raw[8:8 + n]), "sha256_w_u64": sha(raw[8 + n:8 + 9 * n]),
                              "sha256_winv_u64": sha(raw[8 + 9 * n:])}
        res["tables"] = tables
        digits = {}
        for p in DIGIT_EXPONENTS:
            M = (1 << p) - 1
            cases = []
            for v, d in digit_cases(p):
                f = os.path.join(td, "d.bin")
                d.tofile(f)
                res64, eq9, eqMp, zhex, r64d9, r2048d9, r64raw = subprocess.check_output([REF_HOST, "digits", str(p), f]).decode().split()
                case = {"res64": res64, "equal9": int(eq9), "equalMp": int(eqMp), "mpz_sha256": sha(("%x" % int(zhex, 16)).encode()),
                        "res64_div9": r64d9, "res2048_div9": r2048d9, "res64_raw": r64raw, "setmpz_digits": None}
                if v != M:
                    fo = os.path.join(td, "o.bin")
                    subprocess.check_call([REF_HOST, "setmpz", str(p), "%x" % (v + M), fo])
                    case["setmpz_digits"] = int(np.fromfile(fo, dtype=np.uint64).size)
                cases.append(case)
            digits[str(p)] = cases
        res["digits"] = digits
    res["mixed_crt_ll"] = {"%d,%d" % (p, odd): re.sub(r", elapsed [^\n]*", "", subprocess.run([REF_CRT, str(p), str(odd), "--no-progress"],
                                                                                               capture_output=True, text=True, check=True).stdout)
                           for p, odd in LL_CASES}
    path = os.path.join(ROOT, "tests", "golden", "reference_outputs.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
