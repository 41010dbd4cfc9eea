"""The two file formats of prmers_amd/ecm_files.py (no GPU): resume lines against the line the reference publishes for 2^149 - 1
(tests/golden/ecm_resume_p149.p95, copied byte for byte from its docs/), which is a golden vector for the whole stage 1 -- ecm.run on the CPU
oracle must end in its X and CHECKSUM -- every refusal of the parser, and the stage-1 checkpoint: round trip, atomic replacement, and
each CheckpointError."""
import hashlib
import json
import os

import pytest

import orc
from prmers_amd import ecm, ecm_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ecm_resume_p149.p95")
P, SIGMA, B1 = 149, 824476324263488495, 20000
X = 0x1dbfcf8208999587e5713b3c144a12c9a60aa6
CHECKSUM = 1732255967


def fixture_line():
    with open(FIXTURE) as f:
        return f.read()


# ---- resume lines ----

def test_the_fixture_parses_and_its_checksum_verifies():
    line = fixture_line()
    assert F.parse_resume_line(line) == {"p": P, "sigma": SIGMA, "b1": B1, "x": X}
    assert F.checksum(B1, SIGMA, (1 << P) - 1, X) == CHECKSUM and F.CHECKSUM_MODULUS == 4294967291
    # the formula, spelled out
    M = 4294967291
    assert B1 * (SIGMA % M) * (((1 << P) - 1) % M) * (X % M) % M == CHECKSUM
    assert F.read_resume_file(FIXTURE) == [F.parse_resume_line(line)]


def test_resume_line_reproduces_the_fixture_up_to_the_checksum():
    line = fixture_line()
    head = line[:line.index(" PROGRAM=")]
    assert head.startswith("METHOD=ECM; SIGMA=") and head.endswith("CHECKSUM=%d;" % CHECKSUM)
    ours = F.resume_line(P, SIGMA, B1, X, program="someone", time="some day")
    assert ours[:ours.index(" PROGRAM=")] == head
    assert ours[len(head):] == " PROGRAM=someone; X0=0x0; Y0=0x0; TIME=some day;"
    assert F.parse_resume_line(ours) == F.parse_resume_line(line)
    assert "X=0x7;" in F.resume_line(7, 6, 11, 7) and "TIME=" in F.resume_line(7, 6, 11, 7)       # no leading zeros; a time of its own
    with pytest.raises(ValueError):
        F.resume_line(7, 6, 11, 127)                                   # x is a residue


def test_stage_1_on_the_oracle_ends_in_the_fixture_s_x(tmp_path):
    """the whole chain: ecm.suyama, the ladder over ecm.stage1_exponent(20000) on the engine, x = X_Q / Z_Q, the line"""
    out = tmp_path / "p149.p95"
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        res = ecm.run(eng, P, B1, 0, SIGMA, save=str(out))
    assert res["g1"] == 1 and res["x"] == X
    text = out.read_text()
    assert text.endswith(";\n") and text.count("\n") == 1
    assert "X=0x%x; CHECKSUM=%d;" % (X, CHECKSUM) in text
    head = fixture_line()
    assert text.startswith(head[:head.index(" PROGRAM=")] + " PROGRAM=prmers_amd;")
    assert F.read_resume_file(str(out)) == [{"p": P, "sigma": SIGMA, "b1": B1, "x": X}]


def test_fields_in_any_order_unknown_fields_and_the_forms_of_n_x_and_sigma():
    n = (1 << P) - 1
    want = {"p": P, "sigma": SIGMA, "b1": B1, "x": X}
    for line in (
        "X=%d; WHO=me@there; N=%d; CHECKSUM=%d; B1=%d; SIGMA=0x%x; METHOD=ECM; Y=0x0" % (X, n, CHECKSUM, B1, SIGMA),
        "METHOD=ECM; PARAM=0; SIGMA=%d; B1=%d; N=0x%x; X=0x%X;" % (SIGMA, B1, n, X),      # GMP-ECM's own, without a checksum
        "  method=ecm ;sigma=%d;b1=2e4;n=2^149-1;x=0x%x\n" % (SIGMA, X),
        "METHOD=ECM; SIGMA=%d; B1=%d.0; N=2^149 - 1; X=0x%x; CHECKSUM=%d; COMMENT=a=b;" % (SIGMA, B1, X, CHECKSUM),
    ):
        assert F.parse_resume_line(line) == want, line


@pytest.mark.parametrize("change, reason", [
    (("METHOD=ECM", "METHOD=P-1"), "METHOD"),
    (("METHOD=ECM; ", ""), "METHOD"),
    (("METHOD=ECM;", "METHOD=ECM; PARAM=1;"), "PARAM"),
    (("N=2^149-1", "N=%d" % ((1 << 149) + 1)), "2\\^p - 1"),
    (("N=2^149-1", "N=2^149+1"), "N="),
    (("N=2^149-1", "N=2^139-1"), "not below N"),                      # x >= N
    (("X=0x1dbf", "X=0x1dbe"), "CHECKSUM"),                           # a flipped hex digit of X fails on the checksum
    (("X=0x1dbfcf82", "X=0x1dbfcf83"), "CHECKSUM"),
    (("SIGMA=8", "SIGMA=9"), "CHECKSUM"),
    (("CHECKSUM=1732255967", "CHECKSUM=1732255968"), "CHECKSUM"),
    (("B1=20000", "B1=20000.5"), "B1"),
    (("X=0x", "X=0y"), "X="),
    (("SIGMA=824476324263488495; ", ""), "no SIGMA"),
])
def test_every_refusal_says_why(change, reason):
    line = fixture_line()
    assert change[0] in line
    with pytest.raises(F.ResumeFormatError, match=reason):
        F.parse_resume_line(line.replace(change[0], change[1], 1))
    assert issubclass(F.ResumeFormatError, ValueError)


def test_files_skip_blank_and_comment_lines_and_appending_writes_whole_lines(tmp_path):
    path = str(tmp_path / "some.p95")
    a, b = F.resume_line(P, SIGMA, B1, X, time="t"), F.resume_line(127, 11, 50, 12345, time="t")
    F.append_resume_lines(path, [a])
    F.append_resume_lines(path, [])
    F.append_resume_lines(path, [b + "\n", a])
    assert open(path).read() == a + "\n" + b + "\n" + a + "\n"
    with open(path, "a") as f:
        f.write("\n# METHOD=P-1; a comment\n   \n" + b)             # and a last line without its newline
    got = F.read_resume_file(path)
    assert got == [F.parse_resume_line(l) for l in (a, b, a, b)] and got[1] == {"p": 127, "sigma": 11, "b1": 50, "x": 12345}
    with open(path, "a") as f:
        f.write("\nMETHOD=ECM; SIGMA=7; B1=50; N=100; X=1;\n")
    with pytest.raises(F.ResumeFormatError, match="line 8: N is no"):
        F.read_resume_file(path)
    with pytest.raises(ValueError):
        F.append_resume_lines(path, ["two\nlines"])


# ---- checkpoints ----

def header(p=127, sigmas=(6, 7, 8), **kw):
    bits, digest = F.scalar_digest(ecm.stage1_exponent(50))
    h = {"p": p, "b1": 50, "b2": 0, "D": None, "curve": "montgomery", "sigmas": list(sigmas), "substitutes": [1], "scalar_bits": bits,
         "scalar_sha256": digest, "next": 5, "group": 2}
    h.update(kw)
    return h


def registers(p=127, lanes=3):
    mp = (1 << p) - 1
    return [[(r * 1000003 + l + 1) * 0x9E3779B97F4A7C15 ** 3 % mp for l in range(lanes)] for r in range(4)]


def test_a_checkpoint_round_trip_and_the_layout_of_the_file(tmp_path):
    path = str(tmp_path / "a.ckpt")
    F.write_checkpoint(path, header(), registers())
    got, regs = F.read_checkpoint(path)
    assert regs == registers()
    for k, v in header().items():
        assert got[k] == v
    assert (got["version"], got["registers"], got["lanes"], got["word_count"]) == (F.CHECKPOINT_VERSION, 4, 3, 4)
    raw = open(path, "rb").read()
    head, payload = raw.split(b"\n", 1)
    assert json.loads(head) == got and hashlib.sha256(payload).hexdigest() == got["payload_sha256"]
    # the payload: register after register, lane after lane, word_count little-endian 32-bit words each -- what Engine.words_lanes returns
    assert len(payload) == 4 * 3 * 4 * 4
    assert payload[(2 * 3 + 1) * 16:(2 * 3 + 2) * 16] == registers()[2][1].to_bytes(16, "little")
    assert F.scalar_digest(6) == (3, hashlib.sha256(b"\x06").hexdigest())
    # a second write replaces the file as a whole and leaves nothing else behind
    F.write_checkpoint(path, header(next=9), registers())
    assert F.read_checkpoint(path)[0]["next"] == 9 and os.listdir(str(tmp_path)) == ["a.ckpt"]
    # one exponent at which the top word is partly used and one at which it is full
    for p in (149, 160):
        F.write_checkpoint(path, header(p=p, sigmas=(6,)), registers(p, 1))
        assert F.read_checkpoint(path)[1] == registers(p, 1) and F.read_checkpoint(path)[0]["word_count"] == 5
    with pytest.raises(ValueError):
        F.write_checkpoint(path, header(sigmas=(6, 7)), registers())      # one residue per sigma


def test_a_failed_write_leaves_the_old_file(tmp_path, monkeypatch):
    path = str(tmp_path / "a.ckpt")
    F.write_checkpoint(path, header(), registers())
    before = open(path, "rb").read()

    def refuse(src, dst):
        raise OSError("no")
    monkeypatch.setattr(os, "replace", refuse)
    with pytest.raises(OSError):
        F.write_checkpoint(path, header(next=9), registers())
    assert open(path, "rb").read() == before and os.listdir(str(tmp_path)) == ["a.ckpt"]


def test_every_checkpoint_error(tmp_path):
    path = str(tmp_path / "a.ckpt")
    F.write_checkpoint(path, header(), registers())
    raw = open(path, "rb").read()
    cut = raw.index(b"\n") + 1

    def reading(data):
        with open(path, "wb") as f:
            f.write(data)
        return F.read_checkpoint(path)
    assert reading(raw)[1] == registers()
    for data, reason in ((raw[:-1], "short file"), (raw[:cut], "short file"), (raw[:cut - 1], "short file"), (raw[:20], "short file"), (b"", "short file"),
                         (raw + b"\0", "long file"),
                         (raw[:cut + 7] + bytes([raw[cut + 7] ^ 0x10]) + raw[cut + 8:], "SHA-256"),
                         (raw[:-1] + bytes([raw[-1] ^ 1]), "SHA-256"),
                         (raw.replace(b'"version": 1', b'"version": 2', 1), "version"),
                         (raw.replace(b'"version": 1', b'"version": 0', 1), "version"),
                         (b"[1, 2]\n" + raw[cut:], "version"),
                         (b"not json\n" + raw[cut:], "JSON"),
                         (raw.replace(b'"group": 2, ', b"", 1), "lacks group")):
        with pytest.raises(F.CheckpointError, match=reason):
            reading(data)
    assert b'"version": 1' in raw and b'"group": 2, ' in raw
