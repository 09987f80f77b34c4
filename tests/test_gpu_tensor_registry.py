"""-m gpu: sdx_tensor's answers for every id of _abi.T from the compiled library, for the four task kinds with the warm start off
and on.  The body and the literal expected table are tests/tensor_registry_cases.py, shared with tests/test_tensor_registry.py."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import tensor_registry_cases as K       # noqa: E402


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


@pytest.mark.parametrize("warm", K.WARM)
@pytest.mark.parametrize("kind", list(K.KINDS))
def test_tensor_registry(kind, warm):
    K.case_registry(_make, kind, warm)
