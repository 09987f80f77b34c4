"""-m gpu: operational-space (end-effector impedance) torques of the arm through the compiled gfx950 kernels
k_osc_torques<false / true>.  The bodies are tests/osc_cases.py, shared with the emulated run of tests/test_osc.py; N = 3 (one env per
workgroup: no pack size to straddle), and N against 2 N with randomization off and on."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import osc_cases as K                        # noqa: E402


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


BACKEND = (_make, lambda t: t.cuda())


def test_abi_exports_and_argument_errors():
    K.case_abi(BACKEND)


def test_torques_and_wrench_against_float64():
    K.case_against_float64(BACKEND)


def test_damping_at_a_near_singular_arm():
    K.case_near_singular(BACKEND)


def test_task_space_identities():
    K.case_identities(BACKEND)


def test_exact_parts():
    K.case_exact(BACKEND)


def test_link_mass_factors():
    K.case_randomization(BACKEND)


def test_closed_loop_reaches_the_target():
    K.case_closed_loop(BACKEND)


def test_independence_of_the_step():
    K.case_independence(BACKEND)


@pytest.mark.parametrize("randomize", [False, True])
def test_first_n_rows_do_not_depend_on_n(randomize):
    K.case_n_against_2n(BACKEND, randomize)
