"""Engine option "dp_commit_late" on the host-side emulator build (tests/hipemu): both orders of the dp commit give the same
bits, so a commit that moved past its request (a stale register) or in front of the last reader of its LDS tile shows without a GPU."""
import pytest

import dp_commit_late_checks as dc
import engine_checks as ec


@pytest.mark.parametrize("T", [60, 160])
def test_late_commit_is_bit_identical_on_the_emulator(emu_lib, T):
    """T = 60: one tile per window; T = 160: three tiles, the last of block 4 with input rows and no dp rows"""
    dc.check_late_equals_early(emu_lib, ec.DEF, 3, T, grid=2)
