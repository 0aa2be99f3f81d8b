"""A seeded sweep of som_device.split_large_nuclei over size class x dtype pair x layout x min_size kind (0, 15, one
cell exactly on the strict compare) x cell_ids kind (tests/split_nuclei_reference.fuzz_case), every pixel and every table
entry against the numpy statement.  test_split_nuclei.py checks without a GPU that the cases meet every class and that
every one of them contains a split; none is skipped here."""
import numpy as np
import pytest

from tests import split_nuclei_reference as snr
from tests.test_gpu_split_nuclei import check_chain, check_tables

pytestmark = pytest.mark.gpu

BATCH = 10


@pytest.mark.parametrize("first", range(0, snr.N_FUZZ, BATCH))
def test_fuzz_sweep(gpu, first):
    for i in range(first, first + BATCH):
        c = snr.fuzz_case(i)
        want, n = snr.split_vec(c["cell"], c["nuc"], c["cell_ids"], c["min_size"])
        assert n >= 1, i
        check_chain(gpu, c["cell"], c["nuc"], c["cell_ids"], min_size=c["min_size"], layout=c["layout"],
                    force_search=c["force_search"], want=want)
        if i % 3 == 0:
            check_tables(gpu, c["cell"], c["nuc"], layout=c["layout"], force_search=not c["force_search"])
        if i % 10 == 0:                                       # the statement itself against the literal loop
            np.testing.assert_array_equal(want, snr.split_loop(c["cell"], c["nuc"], c["cell_ids"], c["min_size"])[0])
