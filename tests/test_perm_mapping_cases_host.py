"""The oracle of the device's permutation mapping pinned: on every case of tests/perm_mapping_cases.py, at n <= 2^10,
prover.permutation_mapping (numpy + scipy, what tests/test_gpu_perm_mapping.py compares the device with) equals
ref_plonk.permutation_mapping, the independent union-find over Python tuples."""
import numpy as np
import pytest

import ref_plonk as rp
from perm_mapping_cases import SMALL_CASES


@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_host_mapping_equals_the_big_integer_twin(name):
    from halo2_gpu_specific_amd import prover

    ncols, n, copies = SMALL_CASES[name]()
    assert n <= 1 << 10
    want = rp.permutation_mapping(ncols, n, [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in copies])
    map_col, map_row = prover.permutation_mapping(ncols, n, copies)
    assert map_col.shape == map_row.shape == (ncols, n) and map_col.dtype == map_row.dtype == np.uint32
    assert np.array_equal(map_col, np.array([[cell[0] for cell in col] for col in want], dtype=np.uint32).reshape(ncols, n))
    assert np.array_equal(map_row, np.array([[cell[1] for cell in col] for col in want], dtype=np.uint32).reshape(ncols, n))
