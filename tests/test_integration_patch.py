"""The Rust side of the drop-in as verifiable source (VERDICT r1 #8 / missing #4): integration/hip.rs (the `extern "C"`
shim) and integration/halo2_proofs_hip.patch (the `hip` cargo feature re-targeting the reference's call sites).
There is no Rust toolchain, so "verifiable" means: the patch's new modules are the committed shims byte for byte and
are wired in, every `extern "C"` name in hip.rs is an exported symbol of libhalo2_hip.so with the header's argument count,
and the Rust mirror of the evaluate_h descriptor has the C layout.  That the patch applies to the reference tree (and is
what tools/make_hip_patch.py generates from it) needs that tree, which is not part of this repository."""
import os
import re
import subprocess

from h2util import ROOT

PATCH = os.path.join(ROOT, "integration", "halo2_proofs_hip.patch")
HIP_RS = os.path.join(ROOT, "integration", "hip.rs")
EVAL_HIP_RS = os.path.join(ROOT, "integration", "evaluation_hip.rs")
RESIDENT_RS = os.path.join(ROOT, "integration", "hip_resident.rs")


NEW_MODULES = {"halo2_proofs/src/hip.rs": HIP_RS, "halo2_proofs/src/hip_resident.rs": RESIDENT_RS,
               "halo2_proofs/src/plonk/evaluation_hip.rs": EVAL_HIP_RS}
ANY = 'any(feature = "cuda", feature = "hip")'


def _patched_regions():
    """{path: the text of the file after the patch, as far as the patch shows it}: every hunk's context and added lines,
    hunk after hunk (a line of its own between two hunks, so that no pattern spans them)"""
    regions, rel, hunk = {}, None, None
    with open(PATCH) as f:
        for line in f:
            if line.startswith("+++ b/"):
                rel = line[6:].strip()
                regions[rel] = []
            elif line.startswith("--- "):
                rel, hunk = None, None
            elif line.startswith("@@") and rel:
                hunk = []
                regions[rel].append(hunk)
            elif hunk is not None and line[:1] in (" ", "+"):
                hunk.append(line[1:])
    return {rel: "\x00\n".join("".join(h) for h in hunks) for rel, hunks in regions.items()}


def test_patch_creates_the_shims_and_wires_the_call_sites(tmp_path):
    """what the patch does to the reference, read from the patch itself: its new modules (each one hunk from an empty file)
    applied to empty files are the committed shims byte for byte, and the patched regions of the reference's files hold
    the feature, the module declarations, the hip dispatch of every call site and the registration / guard calls of the
    resident polynomials"""
    for rel in NEW_MODULES:
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text("")
    res = subprocess.run(["git", "apply", "--verbose"] + ["--include=" + rel for rel in NEW_MODULES] + [PATCH], cwd=tmp_path,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    for rel, shim in NEW_MODULES.items():
        assert (tmp_path / rel).read_text() == open(shim).read(), rel
    got = _patched_regions()
    src = lambda rel: got["halo2_proofs/src/" + rel]  # noqa: E731
    assert '#[cfg(feature = "hip")]\npub mod hip_resident;' in src("lib.rs")
    assert "hip = []" in got["halo2_proofs/Cargo.toml"]
    arith = src("arithmetic.rs")
    for fn in ("gpu_multiexp_single_gpu_with_bound", "gpu_multiexp_bound", "gpu_multiexp_bound_and_fft", "gpu_fft", "gpu_ifft"):
        assert re.search(r'#\[cfg\(feature = "hip"\)\]\npub fn %s<' % fn, arith), fn
    assert arith.count(ANY) == 2                                                                # both dispatchers
    plonk = src("plonk.rs")
    assert '#[cfg(feature = "hip")]\nmod evaluation_hip;' in plonk
    assert plonk.count(ANY) == 5 and 'feature = "cuda")]' not in plonk.replace(ANY, "")      # plonk.rs:226-240
    ev = src("plonk/evaluation.rs")
    assert '#[cfg(not(%s))]\n    pub(in crate::plonk) fn evaluate_h(' % ANY in ev                # the CPU twin leaves
    assert ev.count("super::evaluation_hip::evaluate_lc(") == 2                                 # evaluate, evaluate_with_theta
    dom = src("poly/domain.rs")
    for call in ("crate::hip::coeff_to_extended(", "crate::hip::extended_to_coeff(", "crate::hip::divide_by_vanishing_poly("):
        assert dom.count(call) == 1, call
    com = src("poly/commitment.rs")
    assert com.count("crate::hip::register_params(&params.g, &params.g_lagrange);") == 2        # unsafe_setup, read
    assert "impl<C: CurveAffine> Drop for Params<C>" in com
    assert "crate::hip::lincomb(&polys, &coeffs)" in src("poly/multiopen/gwc/prover.rs")
    prover = src("plonk/prover.rs")
    assert "crate::hip::device_count().to_string()" in prover
    # resident polynomials: the proving key's coefficient forms are registered at the end of both keygen functions and
    # unregistered by Drop; a proof's advice polynomials by an RAII guard in both create_proof functions
    keygen = src("plonk/keygen.rs")
    assert keygen.count("crate::hip::register_proving_key(&pk);") == 2 and keygen.count("    Ok(pk)\n}") == 2
    assert "impl<C: CurveAffine> Drop for ProvingKey<C>" in plonk and "crate::hip::unregister_proving_key(self);" in plonk
    assert prover.count("let _hip_advice_polys = crate::hip::RegisteredPolys::new(") == 2
    hip = open(HIP_RS).read()
    for name in ("h2_poly_register", "h2_poly_unregister", "pub fn register_proving_key", "pub struct RegisteredPolys", "impl Drop for RegisteredPolys"):
        assert name in hip, name
    # no `feature = "cuda"` gate left alone in the patched regions of the prover's files
    for rel in ("plonk/keygen.rs", "plonk/permutation.rs", "plonk/permutation/keygen.rs", "plonk/permutation/prover.rs", "plonk/prover.rs"):
        left = [l for l in src(rel).splitlines() if 'feature = "cuda"' in l and ANY not in l]
        assert left == [], (rel, left)


def test_shim_declares_only_exported_symbols_with_the_header_arity():
    """every `pub fn h2_*` of hip.rs and hip_resident.rs exists in include/halo2_hip.h with the same number of parameters
    and is exported by the built library"""
    import halo2_gpu_specific_amd as h2

    L = h2.lib()
    header = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = []
    for path, least in ((HIP_RS, 19), (RESIDENT_RS, 25)):
        rs = open(path).read()
        block = rs[rs.index('extern "C" {'):]
        block = block[:block.index("\n}\n")]
        block = re.sub(r"//[^\n]*", "", block)
        found = re.findall(r"pub fn (h2_\w+)\s*\((.*?)\)\s*(?:->\s*[\w\s\*]+)?;", block, flags=re.S)
        assert len(found) >= least, (path, len(found))
        decls += found
    for name, params in decls:
        assert hasattr(L, name), name
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
        assert m, "not in the header: " + name
        c_params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        rs_params = [p for p in params.split(",") if p.strip()]
        assert len(c_params) == len(rs_params), (name, c_params, rs_params)


def test_descriptor_layout_of_the_rust_mirror(tmp_path):
    """`#[repr(C)] H2EvalhDesc` (integration/hip.rs) against `h2_evalh_desc` (include/halo2_hip.h): a C program prints
    offsetof() of every field; names, order, offsets and sizes must be the ones hip.rs declares (H2_EVALH_DESC_OFFSETS,
    *_SIZE), the struct's fields must come in that order with pointer / u32 / [u64; 4] types matching the header, and
    the enum constants must agree"""
    rs = open(HIP_RS).read()
    table = rs[rs.index("pub const H2_EVALH_DESC_OFFSETS"):]
    table = table[:table.index("];")]
    declared = [(m.group(1), int(m.group(2))) for m in re.finditer(r'\("(\w+)", (\d+)\)', table)]
    assert len(declared) >= 40
    header = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    body = header[header.index("typedef struct {\n    uint32_t k, extended_k;"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("} h2_evalh_desc;")], flags=re.S)
    c_fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if not decl:
            continue
        for part in decl.split(","):                      # "const uint64_t *l0", " *l_last", "uint64_t y[4]", " beta[4]"
            c_fields.append(re.findall(r"(\w+)\s*(?:\[\d+\])?\s*$", part.strip())[0])
    assert [n for n, _ in declared] == c_fields, (declared, c_fields)
    # the struct of hip.rs lists the same fields in the same order
    struct = rs[rs.index("pub struct H2EvalhDesc {"):]
    struct = struct[:struct.index("\n}\n")]
    assert re.findall(r"pub (\w+):", struct) == c_fields
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "halo2_hip.h"', "int main(void) {"]
    prog += ['    printf("%s %%zu\\n", offsetof(h2_evalh_desc, %s));' % (n, n) for n in c_fields]
    prog += ['    printf("sizeof %zu %zu %zu\\n", sizeof(h2_evalh_desc), sizeof(h2_value_source), sizeof(h2_calculation));',
             '    printf("enums %d %d %d %d %d %d\\n", H2_VS_INSTANCE, H2_CALC_STORE, H2_CHALLENGE_GAMMA, H2_ANY_INSTANCE, H2_CALC_LC_CHALLENGE, H2_VS_FIXED);',
             "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    got = [(l.split()[0], int(l.split()[1])) for l in lines[:len(c_fields)]]
    assert got == declared
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub const (H2_\w+): (?:usize|u32) = (\d+);", rs)}
    assert lines[len(c_fields)].split()[1:] == [str(consts["H2_EVALH_DESC_SIZE"]), str(consts["H2_VALUE_SOURCE_SIZE"]),
                                                str(consts["H2_CALCULATION_SIZE"])]
    assert lines[len(c_fields) + 1].split()[1:] == [str(consts[n]) for n in ("H2_VS_INSTANCE", "H2_CALC_STORE", "H2_CHALLENGE_GAMMA",
                                                                               "H2_ANY_INSTANCE", "H2_CALC_LC_CHALLENGE", "H2_VS_FIXED")]
