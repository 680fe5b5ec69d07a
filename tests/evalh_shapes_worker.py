"""worker of the evaluate_h shape tests: what has to happen in a process of its own, so that no cache in memory can answer.

  host-cache NAME          (no GPU) the register-budget rebuild of SHAPES[NAME] and its record on disk: h2_evalh_compile returns
                           more stages than h2_evalh_source enumerates, without scratch; the second call finds them on disk; there
                           is one file, whose layout word carries the stage size of the rebuild and the LDS bit; a copy of it with
                           one byte flipped, and one cut short, is a miss and is rebuilt to the same stages
  gpu-reload NAME STAGES   (MI355X) the code objects another process left in H2_JIT_CACHE are loaded, not compiled, in the
                           layout they were rebuilt to, and compute the oracle's bits
Both print one line that starts with "shapes worker ok"."""
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def host_cache(name):
    import evalh_shape_cases as sc
    from h2util import Oracle
    from halo2_gpu_specific_amd import evaluation as ev

    cache = os.environ["H2_JIT_CACHE"]
    kw, claim = sc.build(name, Oracle.get())
    os.environ.update(claim.get("env", {}))
    enumerated = len(sc.layout(kw))
    b = ev.Builder().build(**kw)
    first = ev.compile_only(b)
    assert first["from_cache"] == 0 and first["stages"] > enumerated and first["scratch_bytes"] == 0, (enumerated, first)
    again = ev.compile_only(b)
    assert again["from_cache"] == 2 and again["stages"] == first["stages"] and again["max_registers"] == first["max_registers"], again
    files = os.listdir(cache)
    assert len(files) == 1 and files[0].endswith(".h2ev"), files
    path = os.path.join(cache, files[0])
    good = open(path, "rb").read()
    # magic (6), compiler version (2), layout word, stage count: the stage size the rebuild ended at, and that it moved the
    # arguments to LDS first -- what the reload needs to generate the same stages again
    layout_word, n_stages = struct.unpack_from("<II", good, 8)
    assert good[:6] == b"H2EVG3" and n_stages == first["stages"], (good[:8], n_stages)
    assert layout_word & sc.CACHE_LDS_BIT and 0 < (layout_word & ~sc.CACHE_LDS_BIT) < first["products_per_row"], hex(layout_word)
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x10
    for what, damaged in (("one byte flipped", bytes(flipped)), ("cut short", good[:len(good) // 2])):
        with open(path, "wb") as f:
            f.write(damaged)
        rebuilt = ev.compile_only(b)
        assert rebuilt["from_cache"] == 0 and rebuilt["stages"] == first["stages"], (what, rebuilt)
        assert open(path, "rb").read() == good and os.listdir(cache) == files, what
    print("shapes worker ok: %s enumerated %d compiled %d registers %d layout %#x" % (
        name, enumerated, first["stages"], first["max_registers"], layout_word))


def gpu_reload(name, stages):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
    import numpy as np
    import torch  # noqa: F401  (first: the library binds to torch's HIP runtime)

    import evalh_shape_cases as sc
    from h2util import Oracle
    from halo2_gpu_specific_amd import evaluation as ev

    oracle = Oracle.get()
    kw, claim, want = sc.cached(name, oracle)
    os.environ.update(claim.get("env", {}))
    b = ev.Builder().build(**kw)
    info = ev.prepare(b)
    assert info["from_cache"] == 2 and info["stages"] == stages, info
    before = ev.generated_launches()
    assert np.array_equal(ev.evaluate_h(b), want)
    assert ev.generated_launches() == before + stages
    print("shapes worker ok: %s reloaded %d stages" % (name, stages))


if __name__ == "__main__":
    if sys.argv[1] == "host-cache":
        host_cache(sys.argv[2])
    else:
        gpu_reload(sys.argv[2], int(sys.argv[3]))
