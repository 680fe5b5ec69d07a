"""The package's layering: sibling imports sit at the top of each module (so the import graph is the one the files show), the
host verifier loads without the device prover, and prover.py still hands out every public name -- the owning module's object."""
import ast
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "halo2-gpu-specific_amd")

# (module file, imported sibling) of every relative import inside a function or method body: none.  Params.verify / assert_valid /
# update reach params_check / params_update through params.py's top-level imports; update_params builds its result with
# type(params).from_powers, so neither module needs params.py back.
DEFERRED_SIBLING_IMPORTS = set()

# owning module -> the public names prover.py re-exports from it; a trailing * is a family of constants
SURFACE = {
    "device": ["Device", "footprint", "parse_bytes", "sharding_description", "g1_ntt", "max_scalar_bits"],
    "params": ["Params"],
    "domain": ["Domain", "ROOT_OF_UNITY", "DELTA", "ZETA"],
    "assigned": ["Rational", "resolve_rational", "ASSIGNED_*"],
    "keygen": ["ProvingKey", "keygen", "keygen_from_info", "permutation_mapping", "permutation_mapping_device", "program_descriptor",
               "PM_*", "PERM_MAPPING_SORT_TILE"],
    "cs_format": ["vk_digest"],
    "witness": ["range_check_assigner", "complete_range_check_witness", "complete_range_check_witness_device",
                "range_check_complete_device", "RC_*"],
    "check": ["check_witness", "assert_satisfied", "check_failures", "check_result", "ConstraintNotSatisfied", "Lookup", "Shuffle",
              "Permutation", "CHECK_*"],
    "prover": ["create_proof", "create_proof_with_shplonk", "create_proof_ext", "create_proof_from_witness"],
    "arithmetic": ["OP_*"],
    "transcript": ["R_MOD", "fr_to_mont_limbs"],
    "_lib": ["H2Error", "check"],
    "circuit": ["compile_evaluator"],
}


def _deferred_sibling_imports(path):
    found = set()

    def visit(node, inside):
        if inside and isinstance(node, ast.ImportFrom) and node.level >= 1:
            for alias in node.names:
                found.add((os.path.basename(path), node.module or alias.name))
        inside = inside or isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef))
        for child in ast.iter_child_nodes(node):
            visit(child, inside)

    with open(path) as f:
        visit(ast.parse(f.read(), path), False)
    return found


def test_sibling_imports_sit_at_the_top_of_the_module():
    files = sorted(name for name in os.listdir(PACKAGE) if name.endswith(".py"))
    assert "prover.py" in files and "device.py" in files
    found = set()
    for name in files:
        found |= _deferred_sibling_imports(os.path.join(PACKAGE, name))
    assert found == DEFERRED_SIBLING_IMPORTS


def test_the_host_verifier_loads_without_the_device_prover():
    code = ("import sys\nsys.path.insert(0, %r)\nimport halo2_gpu_specific_amd.verifier\n"
            "print('LOADED', [m for m in ('halo2_gpu_specific_amd.prover', 'halo2_gpu_specific_amd.device', 'torch') "
            "if m in sys.modules])\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "LOADED []" in out.stdout.splitlines(), out.stdout


def test_prover_hands_out_the_owning_modules_objects():
    from halo2_gpu_specific_amd import prover

    for module, names in SURFACE.items():
        owner = importlib.import_module("halo2_gpu_specific_amd." + module)
        for name in names:
            family = [name] if not name.endswith("*") else [n for n in vars(owner) if n.startswith(name[:-1])]
            assert family, (module, name)
            for n in family:
                assert getattr(prover, n) is getattr(owner, n), (module, n)
