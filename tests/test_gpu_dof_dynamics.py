"""-m gpu: joint torques and joint-space dynamics through the compiled gfx950 kernels: k_physics<512 | SDX_PHYS_FORCE>,
k_physics<512 | SDX_PHYS_DR | SDX_PHYS_FORCE> and k_dof_dynamics<false / true>.  The bodies are tests/dof_dynamics_cases.py, shared with the
emulated run of tests/test_dof_dynamics.py; N = 3 (k_dof_dynamics runs one env per workgroup: no pack size to straddle), and N against
2 N for every output of k_dof_dynamics."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import dof_dynamics_cases as K              # noqa: E402


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


BACKEND = (_make, lambda t: t.cuda())


def test_abi_exports_and_argument_errors():
    K.case_abi(BACKEND)


@pytest.mark.parametrize("randomize", [False, True])
def test_off_and_zero_are_bit_identical(golden_dir, randomize):
    K.case_off_and_zero(BACKEND, golden_dir, K.N, randomize)


def test_mass_matrix_against_the_oracle():
    K.case_mass_matrix(BACKEND)


def test_mass_matrix_with_link_mass_factors():
    K.case_mass_matrix(BACKEND, link_factor=[0.7 + 0.035 * k for k in range(K.NL)])


def test_bias_against_the_oracle():
    K.case_bias(BACKEND)


@pytest.mark.parametrize("randomize", [False, True])
def test_drive_against_the_formula(randomize):
    K.case_drive(BACKEND, randomize)


def test_actuation_all_drives_off():
    K.case_actuation_all_off(BACKEND)


@pytest.mark.parametrize("randomize", [False, True])
def test_actuation_arm_off_hand_on_pd(randomize):
    K.case_actuation_arm_off(BACKEND, randomize)


def test_actuation_beyond_the_effort_limit():
    K.case_actuation_clamp(BACKEND)


def test_inverse_dynamics_round_trip():
    K.case_round_trip(BACKEND)


def test_one_shot_and_independence():
    K.case_independence(BACKEND)


@pytest.mark.parametrize("randomize", [False, True])
def test_first_n_rows_do_not_depend_on_n(randomize):
    K.case_n_against_2n(BACKEND, randomize)
