"""The chunk-tabulated constant product (tools/gen_fp_mul.py schedule_chunk -> fp_mul_chunk_dev in csrc/fp_mul_gen.hpp; the
butterfly twiddles of the fixed NTT pass): the logical schedule and its lowered assembly blocks executed with Python
integers, for both fields and both chunk widths, over 2 000 seeded random (x, w) pairs and the corners of either operand.
r = x w (mod p) and r < 2p; a multiply-add emitted as carry-free never carries; no column's accumulator exceeds the bound the
generator claimed for it.  The portable fp_mul_chunk and fp_chunk_table of csrc/field.hpp run over the same operands in a
small host program (tests/fp_mul_chunk_host.cpp, g++)."""
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

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
MAD = re.compile(r"H2_MAD_(FREE|SET|ACC)_[VS]\(([^,]+), ([^)]+)\);")
OMEGA_28 = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C  # of order 2^28 in Fr


def limbs(v):
    return [(v >> (32 * i)) & M32 for i in range(8)]


def table(p, w, cl):
    """the entry fp_chunk_table builds: word l * (8 / cl) + k = limb l of w 2^(32 cl k + 32 (cl + 1)) mod p"""
    nc = 8 // cl
    t = [0] * (8 * nc)
    for k in range(nc):
        for l, v in enumerate(limbs(w * pow(2, 32 * cl * k + 32 * (cl + 1), p) % p)):
            t[l * nc + k] = v
    return t


def operand_pairs(name, p):
    omega_256 = pow(OMEGA_28, 1 << 20, p) if name == "FrParams" else pow(3, (p - 1) // 2, p)  # (Fq: an element of order 2)
    top = (1 << 256) - 1
    xs = [0, 1, p, 2 * p - 1, 4 * p - 1, top] + [top ^ (M32 << (32 * i)) for i in range(8)]
    ws = [0, 1, p - 1, 1 << 253, omega_256]
    rng = random.Random(0xC4 + len(name))
    pairs = [(x, w) for x in xs for w in ws]
    pairs += [(rng.randrange(1 << 256), rng.randrange(p)) for _ in range(2000)]
    return pairs


class Machine:
    """the state a schedule runs on; `value` follows the whole accumulator of the current column"""

    def __init__(self, p, x, t):
        self.mod, self.inv = limbs(p), (-pow(p, -1, 1 << 32)) & M32
        self.a, self.t, self.m = limbs(x), t, {}
        self.lo, self.hi, self.r = 0, 0, [0] * 8
        self.columns = []

    def val(self, tok):
        tok = tok.strip()
        g = re.fullmatch(r"a\.l\[(\d)\]", tok)
        if g:
            return self.a[int(g.group(1))]
        g = re.fullmatch(r"t\.w\[(\d+)\]", tok)
        if g:
            return self.t[int(g.group(1))]
        g = re.fullmatch(r"P::MOD\[(\d)\]", tok)
        if g:
            return self.mod[int(g.group(1))]
        return self.m[tok]

    def line(self, ln):
        """a C line of the schedule, logical (H2_SHIFT*) or lowered; False if it is none of them"""
        g = re.match(r"const uint32_t (m\d) = \(uint32_t\)lo \* P::INV;", ln)
        if g:
            self.m[g.group(1)] = ((self.lo & M32) * self.inv) & M32
        elif re.match(r"r\.l\[\d\] = \(uint32_t\)lo;", ln):
            self.r[int(ln[4])] = self.lo & M32
        elif ln.startswith("H2_SHIFT1") or ln.startswith("lo = (lo >> 32) |"):
            self.columns.append(self.lo | (self.hi << 64))
            self.lo, self.hi = (self.lo >> 32) | (self.hi << 32), 0
        elif ln.startswith("H2_SHIFT0") or ln.startswith("lo >>= 32"):
            self.columns.append(self.lo)   # (hi is not part of this column: nothing in it carried)
            self.lo >>= 32
        else:
            return ln.startswith("//") or not ln
        return True

    def result(self):
        return sum(v << (32 * i) for i, v in enumerate(self.r))


def run(lines, p, x, t):
    mc = Machine(p, x, t)
    for ln in lines:
        ln = ln.strip()
        g = MAD.match(ln)
        if g:
            s = mc.lo + mc.val(g.group(2)) * mc.val(g.group(3))
            carry, mc.lo = s >> 64, s & M64
            if g.group(1) == "FREE":
                assert carry == 0, "a multiply-add emitted as carry-free carried: " + ln
            elif g.group(1) == "SET":
                mc.hi = carry
            else:
                mc.hi += carry
            continue
        assert mc.line(ln), "unparsed schedule line: " + ln
    return mc


def run_lowered(lowered, p, x, t):
    mc = Machine(p, x, t)
    for item in lowered:
        if item[0] != "asm":
            assert mc.line(item[1]), "unparsed line: " + item[1]
            continue
        cy, written, clock = [None] * 3, [None] * 3, 0
        for ins in item[1]:
            if ins[0] == "mad":
                assert cy[ins[4]] in (None, 0), "a pending carry was overwritten"
                s = mc.lo + mc.val(ins[1]) * mc.val(ins[2])
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


@pytest.mark.parametrize("cl", [2, 1])
@pytest.mark.parametrize("name", sorted(gen.FIELDS))
def test_chunk_schedule_and_its_lowered_blocks(name, cl):
    p = gen.FIELDS[name]
    lines, stats = gen.schedule_chunk(p, cl)
    nm = cl + 1
    assert stats["free"] + stats["set"] + stats["acc"] == 64 + 8 * nm
    lowered = gen.lower(lines)
    assert sum(1 for it in lowered if it[0] == "asm" for ins in it[1] if ins[0] == "mad") == 64 + 8 * nm
    claimed = stats["column_max"]
    assert len(claimed) == nm + 8
    for x, w in operand_pairs(name, p):
        t = table(p, w, cl)
        mc = run(lines, p, x, t)
        r = mc.result()
        assert r % p == x * w % p and r < 2 * p, (hex(x), hex(w))
        assert r < p + (p >> 29)
        columns = mc.columns + [mc.lo]
        assert len(columns) == len(claimed)
        assert all(c <= bound for c, bound in zip(columns, claimed)), "a column exceeded the generator's bound"
        low = run_lowered(lowered, p, x, t)
        assert low.result() == r and low.columns == mc.columns


def test_portable_product_and_table_of_field_hpp(tmp_path):
    """fp_chunk_table's entries are the residues the schedule assumes, word for word, and the portable fp_mul_chunk returns what
    the generated schedule does"""
    exe = tmp_path / "fp_mul_chunk_host"
    src = os.path.join(ROOT, "tests", "fp_mul_chunk_host.cpp")
    csrc = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-I", csrc, src, "-o", str(exe)], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-4000:]
    recs, want = bytearray(), []
    for fid, name in enumerate(("FrParams", "FqParams")):
        p = gen.FIELDS[name]
        for cl in (2, 1):
            lines, _ = gen.schedule_chunk(p, cl)
            for x, w in operand_pairs(name, p):
                recs += struct.pack("<II", fid, cl) + x.to_bytes(32, "little") + (w * (1 << 256) % p).to_bytes(32, "little")
                t = table(p, w, cl)
                want.append((t, run(lines, p, x, t).result()))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(bytes(recs))
    res = subprocess.run([str(exe), str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    data = outp.read_bytes()
    assert len(data) == len(want) * 288
    for i, (t, r) in enumerate(want):
        words = struct.unpack_from("<72I", data, 288 * i)
        assert list(words[: len(t)]) == t, ("fp_chunk_table", i)
        assert sum(v << (32 * j) for j, v in enumerate(words[64:])) == r, ("fp_mul_chunk", i)
