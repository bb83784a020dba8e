"""GPU (-m gpu): das_pair2_kernel (csrc/das_pair.hip) on the microphone counts it keeps.  Launches whose microphone count is a
multiple of 32 run das_pair2_cells_kernel (tests/test_cells_pair.py), so the 32- and 64-microphone cases of the older pair tests no
longer reach das_pair2_kernel's halves beyond the second; these do: 48 and 80 microphones (six and ten halves of 8, neither a power
of two), N = 252 (lane 63 stages zeros), 3 frames (the last workgroup row computes its frame twice), rows out of order.  Every map
bit for bit the oracle's, family 8, and bf_last_das_rows() == 1: rows of sample pairs in two shifted copies.
"""
import pytest

from support import nat
from test_cells_pair import Case, maps_and_rows

pytestmark = pytest.mark.gpu

CASES = [
    Case("mics48_n252_f3", 56, 48, 252, 17, 16, 3, 0, 272, False),
    Case("mics80_n252_f3", 90, 80, 252, 17, 16, 3, 0, 272, False),
]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_other_mic_counts_stay_on_pair_rows(nat, oracle_lib, case):
    maps_and_rows(nat, oracle_lib, case, 1)
