"""CPU (-m "not gpu"): sdx_tensor's answers for every id of _abi.T on the emulated simulator (tests/hipemu), for the four task kinds
with the warm start off and on.  The body and the literal expected table are tests/tensor_registry_cases.py, shared with
tests/test_gpu_tensor_registry.py."""
import pytest

torch = pytest.importorskip("torch")

import tensor_registry_cases as K       # noqa: E402
from tests.hipemu.sim import EmuSim     # noqa: E402


@pytest.mark.parametrize("warm", K.WARM)
@pytest.mark.parametrize("kind", list(K.KINDS))
def test_tensor_registry(kind, warm):
    K.case_registry(lambda n, **kw: EmuSim(n, **kw), kind, warm)
