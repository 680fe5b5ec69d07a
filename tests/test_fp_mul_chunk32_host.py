"""The eight-chunk constant product with its table entry taken plane by plane (tools/gen_fp_mul.py lower_planes ->
fp_mul_chunk1_planes_dev / fp_mul_chunk1_splanes_dev in csrc/fp_mul_gen.hpp; the twiddles k_ntt_pass8 keeps in LDS).  Both
lowered forms of schedule_chunk(r, 1) -- table words in vector registers, table words in scalar registers -- are executed
instruction by instruction with Python integers: the carries live in three registers in rotation, none is rewritten while
pending or read before the hazard distance, a table word is read only after its plane was fetched (1 or 2 planes ahead, at
most 2 or 3 planes live), no multiply-add reads two scalar operands.  Over 2 000 seeded random (x, w) pairs and the corners
-- x in {0, 1, p - 1, 4p - 1, 2^256 - 1}, w in {1, p - 1}, and an ENTRY with every limb at its bound (2^32 - 1, the top limb
(p - 1) >> 224: no w produces it, the column bounds assume it) -- the result is congruent to x w (an arbitrary entry: to
sum x_j T_j / 2^64), below p (1 + 2^-29), and equal to the portable fp_mul_chunk<1> of csrc/field.hpp, whose
fp_mul_chunk_planes and fp_chunk_table run in a small host program (tests/fp_mul_chunk32_host.cpp, g++).  The table form
tw_store writes for k_ntt_pass8 (entries 0, 4 .. 124 of the butterfly twiddles) is w 2^(32 j) 2^64 mod p, limb-major."""
import importlib.util
import os
import random
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_fp_mul", os.path.join(ROOT, "tools", "gen_fp_mul.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

P = gen.FIELDS["FrParams"]
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
OMEGA_28 = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C  # of order 2^28 in Fr
BOUND = P + (P >> 29)


def limbs(v):
    return [(v >> (32 * i)) & M32 for i in range(8)]


def entry_of(w):
    """the entry fp_chunk_table<1> builds: word l * 8 + k = limb l of T_k = w 2^(32 k) 2^64 mod p"""
    t = [0] * 64
    for k in range(8):
        for l, v in enumerate(limbs(w * pow(2, 32 * k + 64, P) % P)):
            t[l * 8 + k] = v
    return t


def entry_value(t, x):
    """sum x_k T_k for the entry's residues as they stand"""
    return sum(((x >> (32 * k)) & M32) * sum(t[l * 8 + k] << (32 * l) for l in range(8)) for k in range(8))


ENTRY_AT_BOUND = [M32] * 56 + [(P - 1) >> 224] * 8   # every residue 2^224 ((p - 1) >> 224) + 2^224 - 1: what the column bounds assume
XS = [0, 1, P - 1, 4 * P - 1, (1 << 256) - 1]


def cases():
    """(x, entry, what the result is congruent to times 2^64)"""
    out = []
    for x in XS:
        for w in (1, P - 1):
            out.append((x, entry_of(w)))
        out.append((x, ENTRY_AT_BOUND))
    rng = random.Random(0xC432)
    out += [(x, entry_of(w)) for x, w in ((rng.randrange(1 << 256), rng.randrange(P)) for _ in range(2000))]
    return out


class Machine:
    """the lowered plane-wise schedule on Python integers"""

    def __init__(self, x, t, ahead):
        self.mod, self.inv = limbs(P), (-pow(P, -1, 1 << 32)) & M32
        self.a, self.t, self.m, self.ahead = limbs(x), t, {}, ahead
        self.lo, self.hi, self.r = 0, 0, [0] * 8
        self.planes = {}        # plane -> its eight words, while live
        self.column = None

    def fetch(self, c):
        first = range(self.ahead) if c == 0 else ()
        for q in list(first) + ([c + self.ahead] if c + self.ahead <= 7 else []):
            self.planes[q] = self.t[8 * q: 8 * q + 8]
        for q in [q for q in self.planes if q < c]:
            del self.planes[q]                     # the registers of a finished column's plane are free
        assert len(self.planes) <= self.ahead + 1, "more planes live than the form promises"
        self.column = c

    def val(self, tok, cls):
        """-> (value, whether the operand is a scalar register)"""
        g = re.fullmatch(r"a\.l\[(\d)\]", tok)
        if g:
            return self.a[int(g.group(1))], False
        g = re.fullmatch(r"tp\[(\d)\]\[(\d)\]", tok)
        if g:
            c, k = int(g.group(1)), int(g.group(2))
            assert c == self.column, "a column reads its own plane only"
            assert c in self.planes, "a table word was read before its plane was fetched"
            return self.planes[c][k], cls == "S"
        g = re.fullmatch(r"P::MOD\[(\d)\]", tok)
        if g:
            assert cls == "S"
            return self.mod[int(g.group(1))], True
        return self.m[tok], False

    def line(self, ln):
        g = re.match(r"const uint32_t (m\d) = \(uint32_t\)lo \* P::INV;", ln)
        if g:
            self.m[g.group(1)] = ((self.lo & M32) * self.inv) & M32
        elif re.match(r"r\.l\[\d\] = \(uint32_t\)lo;", ln):
            self.r[int(ln[4])] = self.lo & M32
        elif ln.startswith("lo = (lo >> 32) |"):
            self.lo, self.hi = (self.lo >> 32) | (self.hi << 32), 0
        elif ln.startswith("lo >>= 32"):
            self.lo >>= 32
        else:
            return ln.startswith("//") or not ln
        return True

    def result(self):
        return sum(v << (32 * i) for i, v in enumerate(self.r))


def run_lowered(lowered, x, t, ahead, table_cls):
    mc = Machine(x, t, ahead)
    for item in lowered:
        if item[0] == "fetch":
            mc.fetch(item[1])
            continue
        if item[0] != "asm":
            assert mc.line(item[1]), "unparsed line: " + item[1]
            continue
        cy, written, clock = [None] * 3, [None] * 3, 0
        for ins in item[1]:
            if ins[0] == "mad":
                assert cy[ins[4]] in (None, 0), "a pending carry was overwritten"
                (xv, xs), (yv, ys) = mc.val(ins[1], "V"), mc.val(ins[2], ins[3])
                assert not xs and (ys == (ins[3] == "S")), "operand class"
                assert xs + ys <= 1, "two scalar operands in one multiply-add"
                if ins[2].startswith("tp["):
                    assert ins[3] == table_cls
                s = mc.lo + xv * yv
                cy[ins[4]], mc.lo, written[ins[4]] = s >> 64, s & M64, clock
                clock += 1
            elif ins[0] == "nop":
                clock += ins[1]
            else:
                assert clock - written[ins[1]] - 1 >= gen.WAIT, "carry read too early"
                mc.hi = cy[ins[1]] if ins[0] == "set" else mc.hi + cy[ins[1]]
                cy[ins[1]], written[ins[1]] = None, None
                clock += 1
        assert all(c in (None, 0) for c in cy), "a carry was dropped at the end of a block"
    return mc


def run_logical(lines, x, t):
    """the schedule's macro lines (what tests/test_fp_mul_chunk_schedule.py executes), for the expected value"""
    lo = hi = 0
    a, mod, inv, m, r = limbs(x), limbs(P), (-pow(P, -1, 1 << 32)) & M32, {}, [0] * 8
    for ln in lines:
        ln = ln.strip()
        g = re.match(r"H2_MAD_(FREE|SET|ACC)_[VS]\(([^,]+), ([^)]+)\);", ln)
        if g:
            def val(tok):
                tok = tok.strip()
                if tok.startswith("a.l["):
                    return a[int(tok[4])]
                if tok.startswith("t.w["):
                    return t[int(tok[4:-1])]
                if tok.startswith("P::MOD["):
                    return mod[int(tok[7])]
                return m[tok]
            s = lo + val(g.group(2)) * val(g.group(3))
            hi, lo = (s >> 64 if g.group(1) == "SET" else hi + (s >> 64)), s & M64
        elif ln.startswith("const uint32_t m"):
            m[ln.split()[2]] = ((lo & M32) * inv) & M32
        elif ln.startswith("r.l["):
            r[int(ln[4])] = lo & M32
        elif ln.startswith("H2_SHIFT1"):
            lo, hi = (lo >> 32) | (hi << 32), 0
        elif ln.startswith("H2_SHIFT0"):
            lo >>= 32
        else:
            assert ln.startswith("//") or not ln, ln
    return sum(v << (32 * i) for i, v in enumerate(r))


@pytest.fixture(scope="module")
def expected():
    lines, _ = gen.schedule_chunk(P, 1)
    return [(x, t, run_logical(lines, x, t)) for x, t in cases()]


def test_the_expected_values_are_the_product(expected):
    inv64 = pow(1 << 64, -1, P)
    for x, t, r in expected:
        assert r % P == entry_value(t, x) * inv64 % P and r < BOUND, hex(x)
    corners = {(x, tuple(t)): r for x, t, r in expected[: 3 * len(XS)]}
    for x in XS:
        for w in (1, P - 1):
            assert corners[(x, tuple(entry_of(w)))] % P == x * w % P, (hex(x), hex(w))
    rng = random.Random(0xC432)     # (the random pairs again, as cases() drew them: congruent to x w itself)
    for x, _, r in expected[3 * len(XS):]:
        xx, w = rng.randrange(1 << 256), rng.randrange(P)
        assert xx == x and r % P == x * w % P


@pytest.mark.parametrize("ahead", [1, 2])
@pytest.mark.parametrize("cls", ["V", "S"])
def test_the_lowered_forms_instruction_by_instruction(expected, cls, ahead):
    lines, stats = gen.schedule_chunk(P, 1)
    assert (stats["free"], stats["set"], stats["acc"]) == (16, 8, 56)
    lowered = gen.lower_planes(lines, cls)
    mads = [ins for it in lowered if it[0] == "asm" for ins in it[1] if ins[0] == "mad"]
    assert len(mads) == 80 and sum(1 for ins in mads if ins[2].startswith("tp[")) == 64
    assert [it[1] for it in lowered if it[0] == "fetch"] == list(range(8))
    for x, t, want in expected:
        got = run_lowered(lowered, x, t, ahead, cls).result()
        assert got == want and got < BOUND, (hex(x), cls, ahead)


def test_the_header_holds_what_the_generator_emits():
    """fp_mul_gen.hpp is regenerated, not edited: both plane-wise functions are there, text for text"""
    lines, _ = gen.schedule_chunk(P, 1)
    with open(os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc", "fp_mul_gen.hpp")) as f:
        header = f.read()
    for cls, fn in (("V", "fp_mul_chunk1_planes_dev"), ("S", "fp_mul_chunk1_splanes_dev")):
        body = "\n".join(gen.emit(gen.lower_planes(lines, cls)))
        assert fn in header and body in header, fn
    assert '"s"(tp[' in "\n".join(gen.emit(gen.lower_planes(lines, "S")))
    assert '"s"(tp[' not in "\n".join(gen.emit(gen.lower_planes(lines, "V")))


def test_portable_planes_product_and_the_pass_table(tmp_path, expected):
    """csrc/field.hpp on the host: fp_mul_chunk_planes over a plane fetch returns what the schedule does (and so does the
    portable fp_mul_chunk<1> it wraps), and fp_chunk_table<1> -- what tw_store's fourth form writes, 16-byte word by word --
    gives w 2^(32 j) 2^64 mod p, limb-major, for the 32 indices 0, 4 .. 124 of a 2^8-point pass's butterfly twiddles"""
    exe = tmp_path / "fp_mul_chunk32_host"
    src = os.path.join(ROOT, "tests", "fp_mul_chunk32_host.cpp")
    csrc = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-I", csrc, src, "-o", str(exe)], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-4000:]
    # records: kind 0 = (x, entry) -> product; kind 1 = (w in Montgomery form) -> entry
    recs = bytearray()
    for x, t, _ in expected:
        recs += struct.pack("<I", 0) + x.to_bytes(32, "little") + struct.pack("<64I", *t)
    w256 = pow(OMEGA_28, 1 << 20, P)    # the butterfly root of an 8-bit pass
    ws = [pow(w256, 4 * i, P) for i in range(32)]
    for w in ws:
        recs += struct.pack("<I", 1) + (w * (1 << 256) % P).to_bytes(32, "little") + bytes(256)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(bytes(recs))
    res = subprocess.run([str(exe), str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    data = outp.read_bytes()
    assert len(data) == (len(expected) + len(ws)) * 256
    for i, (x, t, want) in enumerate(expected):
        r = struct.unpack_from("<16I", data, 256 * i)
        assert sum(v << (32 * j) for j, v in enumerate(r[:8])) == want, ("fp_mul_chunk_planes", i)
        assert sum(v << (32 * j) for j, v in enumerate(r[8:])) == want, ("fp_mul_chunk<1>", i)
    for i, w in enumerate(ws):
        words = struct.unpack_from("<64I", data, 256 * (len(expected) + i))
        assert list(words) == entry_of(w), ("fp_chunk_table<1>", 4 * i)
        for j in range(8):
            assert sum(words[l * 8 + j] << (32 * l) for l in range(8)) == w * pow(2, 32 * j + 64, P) % P
