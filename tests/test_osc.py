"""CPU (-m "not gpu"): operational-space (end-effector impedance) torques of the arm (include/seqdex.h sdx_osc_torques) on
the SIMT emulator: k_osc_torques<false / true> compiled by g++.

- the ABI: the export, every argument error, version 8 and 56 tensor ids, the Python tensor checks;
- torques and wrench against the law in numpy float64, also at a near-singular arm and with link mass factors;
- the two task-space identities, the exact parts (zeros, the bias, the clamp);
- the closed loop through the unchanged physics step, and the call's independence of the step.
The bodies are tests/osc_cases.py, shared with tests/test_gpu_osc.py."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

import osc_cases as K                        # noqa: E402
from seqdex_amd import _abi                  # noqa: E402
from tests.hipemu.sim import EmuSim          # noqa: E402


class EmuOscSim(EmuSim):
    """the emulated simulator with the prototypes of the new call and of the two it is used with (tests/hipemu declares those of the calls it
    wraps itself)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        vp = C.c_void_p
        self.lib.sdx_osc_torques.argtypes = [vp, C.POINTER(_abi.OscAttr), vp, vp, vp, vp]
        self.lib.sdx_apply_dof_forces.argtypes = [vp, vp, C.c_uint32, vp]
        self.lib.sdx_dof_dynamics.argtypes = [vp, vp, vp, vp, vp]


BACKEND = (EmuOscSim, lambda t: t)


def test_abi_exports_and_argument_errors():
    K.case_abi(BACKEND)


def test_gains_and_pose_error():
    K.case_gains_and_pose_error()


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
