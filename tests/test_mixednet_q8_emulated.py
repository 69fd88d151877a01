"""int8 streaming evaluation of MixedNets with residual connections or a pooled head (stream_q8_kernel<true> of csrc/tu_stream_q8.hip,
mww_stream_create_mixednet_q8) under the host-side emulator of tests/hipemu: every case of tests/quant_mixednet_checks.py -
calibration on the device, then outputs, logits and rings bit for bit against tests/quant_mixednet_oracle.py - and the ABI."""
import pytest

import quant_mixednet_checks as mc


@pytest.mark.parametrize("cid", mc.case_ids())
def test_case_equals_the_oracle_bit_for_bit(emu_lib, cid):
    res = mc.run_case(emu_lib, cid, n_cu=4)   # the emulated device has 4 CUs
    print("[mixednet_q8] %s" % res, flush=True)


def test_abi(emu_lib):
    mc.check_abi(emu_lib)
