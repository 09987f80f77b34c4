"""CPU (-m "not gpu"): external forces and torques on rigid bodies and the random pushes on the target brick (DESIGN.md section 21,
include/seqdex.h sdx_apply_rigid_body_forces / sdx_set_force_perturbation) on the SIMT emulator.

- the ABI: exports, the struct mirror, argument errors;
- off and zero: an all-zero wrench and a forgotten one-shot wrench against no call at all, bit for bit;
- closed forms in free flight, the gravity equivalence on contact-rich piles, robot links against J^T w;
- the sampler (sdx_randomize.hip k_force_perturb) against the numpy restatement of tests/helpers/force_perturb_restatement.py.
The bodies are tests/rigid_body_force_cases.py, shared with tests/test_gpu_rigid_body_forces.py."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from seqdex_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3


def test_exports_and_struct_layout():
    src = ('#include <stdio.h>\n#include "seqdex.h"\nint main(){printf("%zu %d %d %d\\n", sizeof(sdx_force_perturb_attr), SDX_ABI_VERSION, '
           '(int)SDX_SPACE_ENV, (int)SDX_SPACE_LOCAL);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        size, abi, env, local = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert size == C.sizeof(_abi.ForcePerturbAttr) == 20
    assert abi == _abi.SDX_ABI_VERSION == 8 and len(_abi.T) == 56            # no tensor id, no version bump
    assert (env, local) == (_abi.SPACE_ENV, _abi.SPACE_LOCAL)
    assert "sdx_apply_rigid_body_forces" in _abi.SDX_EXPORTS and "sdx_set_force_perturbation" in _abi.SDX_EXPORTS


torch = pytest.importorskip("torch")

import rigid_body_force_cases as K          # noqa: E402
from tests.hipemu.sim import EmuSim          # noqa: E402


class EmuForceSim(EmuSim):
    """the emulated simulator with the prototypes of the two new calls (tests/hipemu declares those of the calls it wraps itself)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        vp = C.c_void_p
        self.lib.sdx_apply_rigid_body_forces.argtypes = [vp, vp, vp, C.c_int32, vp]
        self.lib.sdx_set_force_perturbation.argtypes = [vp, C.POINTER(_abi.ForcePerturbAttr), vp, vp, vp]


BACKEND = (EmuForceSim, lambda t: t)


def test_argument_errors():
    K.case_abi_errors(BACKEND)


@pytest.mark.parametrize("randomize", [False, True])
def test_off_and_zero_wrench_are_bit_identical(golden_dir, randomize):
    K.case_off_and_zero(BACKEND, golden_dir, N, randomize)


def test_free_flight_closed_forms():
    K.case_free_flight(BACKEND, N)


def test_gravity_equivalence_on_piles(golden_dir):
    K.case_gravity_equivalence(BACKEND, golden_dir, N)


@pytest.mark.parametrize("space,factor", [("env", None), ("local", None), ("env", 1.4)])
def test_robot_links_against_the_jacobian(space, factor):
    K.case_robot_links(BACKEND, space, factor)


@pytest.mark.parametrize("randomize", [False, True])
def test_sampler_against_the_restatement(randomize):
    K.case_sampler(BACKEND, 8, randomize)


def test_sampler_does_not_depend_on_n():
    K.case_sampler_independent_of_n(BACKEND, 8, 16)


def test_sampler_snapshot_replays_the_pushes():
    K.case_sampler_snapshot(BACKEND, 8)


def test_step_applies_the_pushes_and_replaces_the_callers_wrench():
    K.case_step_applies_the_pushes(BACKEND, N)
