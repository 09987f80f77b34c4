"""CPU (-m "not gpu"): joint torques and joint-space dynamics (include/seqdex.h sdx_apply_dof_forces /
sdx_dof_dynamics) on the SIMT emulator: the k_physics<.. | SDX_PHYS_FORCE> instantiations and k_dof_dynamics compiled by g++.

- the ABI: exports, argument errors, version 8 and 56 tensor ids;
- off and zero: zero DOF forces and a consumed one-shot call against no call at all, bit for bit;
- mass matrix, bias and drive against the C oracle, a float64 CRBA and the numpy formula;
- actuation against the unchanged oracle (torque sources stated through soft gains), the inverse-dynamics round trip;
- the pending slot's independence of the wrench, the sampler and snapshots.
The bodies are tests/dof_dynamics_cases.py, shared with tests/test_gpu_dof_dynamics.py."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

import dof_dynamics_cases as K               # noqa: E402
from seqdex_amd import _abi                  # noqa: E402
from tests.hipemu.sim import EmuSim          # noqa: E402


class EmuDofSim(EmuSim):
    """the emulated simulator with the prototypes of the two new calls, and of the wrench calls the independence test makes (tests/hipemu
    declares those of the calls it wraps itself)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        vp = C.c_void_p
        self.lib.sdx_apply_dof_forces.argtypes = [vp, vp, C.c_uint32, vp]
        self.lib.sdx_dof_dynamics.argtypes = [vp, vp, vp, vp, vp]
        self.lib.sdx_apply_rigid_body_forces.argtypes = [vp, vp, vp, C.c_int32, vp]
        self.lib.sdx_set_force_perturbation.argtypes = [vp, C.POINTER(_abi.ForcePerturbAttr), vp, vp, vp]


BACKEND = (EmuDofSim, lambda t: t)


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
    """measured on the emulator: the oracle's quadratic defect 8.9e-06 N m (bar 3.5e-05), engine - oracle 1.9e-05 N m, largest |bias| 7.7 N m"""
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


def test_pd_torques_restate_the_reference_law():
    K.case_pd_torques()


def test_one_shot_and_independence():
    K.case_independence(BACKEND)
