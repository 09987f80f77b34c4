"""The tensor registry of the PPO library (include/seqdex.h sdxp_tensor): every id of _abi.TP must come back with the dtype, ndim and
shape of the literal table below and a non-null pointer, for 4 actors x horizon 8 in four configurations - the shipped minibatch 4,
minibatch 16 (the GEMM path: the rank-MB factor buffers shrink to one row), world_size 2 (FACTORS_ALL grows a rank) and obs_dim 186
(network input padded to 188, obs_cols 186).  The table was not produced by the code under test: it is the dump of the commit BEFORE
the registry became a table (profiles/ppo_units_tensor_registry_parent.txt), whose registry was 27 hand-written lines."""
import ctypes as C

import pytest

from seqdex_amd import _abi

pytestmark = pytest.mark.gpu

F32, I64, F64 = 0, 1, 4        # sdx_dtype codes of include/seqdex.h
P_AC, P_CV = 2131503, 1234945  # parameters of the actor-critic (obs 396) and of the central-value network (state 564)

# the shipped minibatch 4
BASE = {
    "AC_PARAMS": (F32, [P_AC]), "AC_GRADS": (F32, [P_AC]), "CV_PARAMS": (F32, [P_CV]), "CV_GRADS": (F32, [P_CV]),
    "MB_OBS": (F32, [4, 8, 396]), "MB_STATES": (F32, [4, 8, 564]), "MB_ACTIONS": (F32, [4, 8, 23]), "MB_MUS": (F32, [4, 8, 23]),
    "MB_SIGMAS": (F32, [4, 8, 23]), "MB_NEGLOGP": (F32, [4, 8]), "MB_VALUES": (F32, [4, 8]), "MB_REWARDS": (F32, [4, 8]),
    "MB_DONES": (F32, [4, 8]), "RETURNS": (F32, [32]), "ADVANTAGES": (F32, [32]), "CV_RMS_MEAN": (F64, [564]), "CV_RMS_VAR": (F64, [564]),
    "STATS": (F32, [636]), "LAST_VALUES": (F32, [4]), "AC_ADAM_M": (F32, [P_AC]), "AC_ADAM_V": (F32, [P_AC]), "CV_ADAM_M": (F32, [P_CV]),
    "CV_ADAM_V": (F32, [P_CV]), "DEBUG": (I64, [64]), "ALL_GRADS": (F32, [3366592]), "FACTORS": (F32, [48640]), "FACTORS_ALL": (F32, [1, 48640]),
}
P_AC_186 = 1705519
# configuration -> (arguments of make_config, what it changes of the table, parameters of the actor-critic)
CASES = {
    "minibatch_4": (dict(), {}, P_AC),
    "minibatch_16": (dict(params={"config": {"minibatch_size": 16}}), {"FACTORS": (F32, [12224]), "FACTORS_ALL": (F32, [1, 12224])}, P_AC),
    "world_size_2": (dict(world_size=2), {"FACTORS_ALL": (F32, [2, 48640])}, P_AC),
    "obs_dim_186": (dict(obs_dim=186), dict({k: (F32, [P_AC_186]) for k in ("AC_PARAMS", "AC_GRADS", "AC_ADAM_M", "AC_ADAM_V")},
                                            MB_OBS=(F32, [4, 8, 188]), ALL_GRADS=(F32, [2940608]), FACTORS=(F32, [46976]),
                                            FACTORS_ALL=(F32, [1, 46976])), P_AC_186),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_id_has_the_parents_dtype_shape_and_a_pointer(case):
    from seqdex_amd.ppo import SdxPPO, make_config
    kw, changes, p_ac = CASES[case]
    assert set(BASE) == set(_abi.TP) and len(_abi.TP) == 27
    want = dict(BASE)
    want.update(changes)
    cfg = make_config(4, **kw)
    assert (cfg.horizon, cfg.obs_dim, cfg.obs_cols) == ((8, 188, 186) if case == "obs_dim_186" else (8, 396, 0))
    p = SdxPPO(4, config=cfg)
    try:
        assert p.update_impl() == ("gemm" if case == "minibatch_16" else "persistent")
        ptrs = {}
        for name, tid in _abi.TP.items():
            ptr, shape, ndim, dt = C.c_void_p(), (C.c_int64 * 4)(), C.c_int32(), C.c_int32()
            p._check(p.lib.sdxp_tensor(p.h, tid, C.byref(ptr), shape, C.byref(ndim), C.byref(dt)))
            shape = [shape[i] for i in range(4)]
            w_dtype, w_shape = want[name]
            assert (dt.value, ndim.value, shape[:ndim.value]) == (w_dtype, len(w_shape), w_shape), (case, name)
            assert shape[ndim.value:] == [1] * (4 - ndim.value), (case, name)          # the words past ndim are 1
            assert ptr.value, (case, name)
            ptrs[name] = ptr.value
        # both flat gradients and the KL word are one allocation: [ac_g | pad to 64 | cv_g | pad to 64 | 64 words]
        assert ptrs["ALL_GRADS"] == ptrs["AC_GRADS"], case
        assert ptrs["CV_GRADS"] - ptrs["AC_GRADS"] == 4 * ((p_ac + 63) // 64 * 64), case
    finally:
        p.close()
