"""Shared body of the tensor registry tests (include/seqdex.h sdx_tensor): tests/test_tensor_registry.py runs it on the emulated
simulator (tests/hipemu), tests/test_gpu_tensor_registry.py on the GPU.  For the four task kinds, with the warm start off and on, at
N = 3 (odd, no multiple of 4, the smallest N at which the N x actors row shapes differ from N), every id of _abi.T must come back with the
dtype, ndim and shape of the literal table below and a non-null pointer.  The table was not produced by the code under test: it is the
dump of the commit BEFORE the buffer table (profiles/buffer_table_tensor_registry_parent.txt), whose registry was 56 hand-written lines.
Orient and Search use the default pile ring of 512 slots."""
import ctypes as C

from seqdex_amd import _abi

N = 3
F32, I64, I32, I16 = 0, 1, 2, 5        # sdx_dtype codes of include/seqdex.h
KINDS = {"grasp": dict(), "orient": dict(task_kind=1), "insert": dict(task_kind=2, max_episode_length=125.0),
         "search": dict(task_kind=3, max_episode_length=75.0, act_moving_average=0.6, target_euler=[0.0, 3.14, 1.57])}
WARM = (0.0, 0.8)

# GraspSim, warm start off
BASE = {
    "ROOT": (F32, [426, 13]), "DOF": (F32, [69, 2]), "RB": (F32, [3, 165, 13]), "CONTACT": (F32, [3, 495]), "JAC_EEF": (F32, [3, 6, 7]),
    "TARGETS": (F32, [3, 23]), "PREV_TARGETS": (F32, [3, 23]), "OBS": (F32, [3, 396]), "STATES": (F32, [3, 564]),
    "OBS_CLAMPED": (F32, [3, 396]), "STATES_CLAMPED": (F32, [3, 564]), "REW": (F32, [3]), "RESET": (I64, [3]), "PROGRESS": (I64, [3]),
    "RANDOMIZE": (I64, [3]), "ACTIONS": (F32, [3, 23]), "INIT_POS": (F32, [3, 3]), "INIT_ROT": (F32, [3, 4]), "SUCCESSES": (F32, [3]),
    "META_REW": (F32, [3]), "CONS_SUCCESSES": (F32, [1]), "FINGER_DIST": (F32, [3]), "TVALUE": (F32, [3]), "ARM_CONTACTS": (F32, [3, 6]),
    "STUDENT_OBS": (F32, [3, 30]), "SUCCESS_BUF": (I64, [3]), "PILE_CHOICE": (I32, [3]), "NCONTACTS": (I32, [3]), "DEBUG": (I64, [70]),
    "HARVEST_HAND": (F32, [8, 5001, 23, 2]), "HARVEST_OBJ": (F32, [8, 5001, 13]), "HARVEST_COUNT": (I32, [8]), "INSERT_AUX": (F32, [3, 8]),
    "TV_SUCCESS": (F32, [1048576, 4]), "TV_FAILURE": (F32, [1048576, 4]), "TV_COUNT": (I32, [2]), "PILE_HARVEST": (F32, [8, 1, 132, 13]),
    "PILE_HARVEST_COUNT": (I32, [8]), "SEG_IMAGE": (I16, [1, 1, 1]), "SEG_PIXELS": (F32, [3, 4]), "EMERGENCE": (F32, [3]),
    "JACOBIAN": (F32, [3, 23, 6, 23]), "TVALUE_OBS": (F32, [1, 1]), "CONTACT_STATS": (I32, [4]), "WARM_COUNT": (I32, [3]),
    "CAM_ROT": (F32, [3, 4]), "TV_KEYS": (I64, [2, 1048576]), "HARVEST_KEYS": (I64, [8, 5001]), "PILE_HARVEST_KEYS": (I64, [8, 1]),
    "WARM_KEYS": (I32, [1]), "WARM_LAMBDA": (F32, [1]), "DR_DOF": (F32, [3, 4, 23]), "DR_LINK": (F32, [3, 2, 24]),
    "DR_BRICK": (F32, [3, 2, 72]), "DR_GRAVITY": (F32, [3]), "DR_FRAME": (I64, [2]),
}
# what the other configurations change of it
PILE_RING = {"PILE_HARVEST": (F32, [8, 512, 132, 13]), "PILE_HARVEST_KEYS": (I64, [8, 512])}
BY_KIND = {
    "grasp": {},
    "orient": dict(PILE_RING, OBS=(F32, [3, 186]), OBS_CLAMPED=(F32, [3, 186])),
    "insert": dict(OBS=(F32, [3, 75]), OBS_CLAMPED=(F32, [3, 75])),
    "search": dict(PILE_RING, OBS=(F32, [3, 186]), OBS_CLAMPED=(F32, [3, 186]), SEG_IMAGE=(I16, [3, 128, 128]), TVALUE_OBS=(F32, [3, 652])),
}
WARM_ON = {"WARM_KEYS": (I32, [3, 1536]), "WARM_LAMBDA": (F32, [3, 3, 1536])}


def expected(kind, warm):
    want = dict(BASE)
    want.update(BY_KIND[kind])
    if warm > 0:
        want.update(WARM_ON)
    return want


def query(sim, tid):
    """sdx_tensor as the library answers it: (pointer, dtype, ndim, the four shape words)"""
    ptr, shape, ndim, dt = C.c_void_p(), (C.c_int64 * 4)(), C.c_int32(), C.c_int32()
    sim._check(sim.lib.sdx_tensor(sim.h, tid, C.byref(ptr), shape, C.byref(ndim), C.byref(dt)))
    return ptr.value, dt.value, ndim.value, [shape[i] for i in range(4)]


def case_registry(make, kind, warm):
    assert set(BASE) == set(_abi.T) and len(_abi.T) == 56
    want = expected(kind, warm)
    s = make(N, warm_start=warm, **KINDS[kind])
    try:
        ptrs = {}
        for name, tid in _abi.T.items():
            ptr, dtype, ndim, shape = query(s, tid)
            w_dtype, w_shape = want[name]
            assert (dtype, ndim, shape[:ndim]) == (w_dtype, len(w_shape), w_shape), (kind, warm, name)
            assert shape[ndim:] == [1] * (4 - ndim), (kind, warm, name)          # the words past ndim are 1
            assert ptr, (kind, warm, name)
            ptrs[name] = ptr
        # the temporal buffer belongs to Search: everywhere else SDX_T_TVALUE_OBS is a {1, 1} view of SDX_T_SEG_PIXELS
        assert (ptrs["TVALUE_OBS"] == ptrs["SEG_PIXELS"]) == (kind != "search"), (kind, warm)
    finally:
        s.close()
