"""-m gpu: the persistent update takes the 4x4 Grams of its layer-0 inputs from a per-epoch table.  The inputs of a step are dataset rows
(observations; the central value's rows as the pre-normalisation left them, class cvx0 for mini-epoch 0 and cvx1 afterwards), so their Grams do
not depend on the step: k_input_grams (csrc/sdxp_persist.hip) forms every minibatch's once per epoch, behind the pre-normalisation, and
k_update_persistent<false> fetches the 32 floats of its minibatch with the rows instead of reducing them in the shadow of its x1 edge.  The Grams
enter the squared gradient norm (<G_dY0, G_x0>), hence the clip scale and every parameter: the table must hold the BITS the in-kernel form had.
That form is kept as the test entry sdxpk_input_grams_reference (csrc/sdxp_persist_checks.hip: rows in the S.obs / S.cvx images, gram_acc10,
block_sum<22>, built with the epoch kernel's flags).

(a) table against reference, bit for bit, all 3 x 16 entries of 8 minibatches, observation widths 396 and 188 (Orient's; the tail columns of the
    image are zero) beside the 564 wide state rows; inputs of helpers/input_gram_cases.py (wide dynamic range, an all-zero row, a column that is
    negative in all rows).  First the reference is shown to differ from a plain ascending float32 sum in more than half of its entries: a table
    that summed in another order could not pass by accident.
(b) reference against float64 on the host: every entry within 40 * 2^-24 * sum_k |a_k b_k| - along any path a term meets at most 2 per-thread
    roundings (product, fma of the second column), 4 butterfly levels and 32 row adds, 38 in all; every diagonal entry greater than zero
    (but the one of the all-zero row, which must be +0.0).
(c) the right matrix reaches the right step: 8 minibatches (N = 4 x horizon 8), normalize_input on, so cvx0 != cvx1; mini_epochs 1 and 2; after
    update() the control block's ac_gnorm / cv_gnorm - the norm of the LAST step, which lies in mini-epoch 0 and in mini-epoch 1 respectively -
    of the persistent path against impl="graph", which forms its own norms.  (Adam is nearly scale-invariant: a wrong Gram barely shows in the
    parameters, the norm shows it directly.)  Relative differences between the two paths measured with measure_paths() on the commit BEFORE this
    change, same seeds:

        mini_epochs 1: actor-critic persistent 13.1384583 graph 13.1384335 .. 13.1384325 -> 1.9598e-06, central value 2.25028038 / 2.25028086 .. 2.25029063 -> 4.5559e-06
        mini_epochs 2: actor-critic persistent 1.3544451  graph 1.35444462 .. 1.35444486 -> 3.5205e-07, central value 16.6559963 / 16.6559849 .. 16.6560077 -> 6.8709e-07

    The persistent path's norms are the same bits in every run; the hipGraph path's move in their seventh digit from run to run (its reductions
    use atomics), so each figure is the LARGEST of 72 measurements on the parent commit.
    The test allows four times these figures.  What a wrong matrix would do, measured with measure_wrong_class() (float64 on the host, the
    central value's factors of minibatch 0 at the initial parameters from the one-minibatch kernel, the Gram of the minibatch's cvx0 rows
    replaced by the Gram of its cvx1 rows, which the host restates from the states and the running statistics):

        norm with the Gram of the cvx0 rows 5.51558361, with the Gram of the cvx1 rows 6.2988453: a move of 1.42e-01, 13 000 times the widest
        bound (1.8e-05).  The persistent path's own figures of this tree are the parent's to the last bit.

(d) two persistent handles from one state at N = 16 x horizon 8 (160 steps, four mini-epoch wraps of the row prefetch): parameters, Adam moments
    and the rewritten mu / sigma rows bit-identical - the table's 32 floats arrive through the same global_load_lds and the same wait as the
    rows, nothing may depend on timing."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers.input_gram_cases import MB, N_MB, ST, bits, gram_ascending, gram_float64, rows  # noqa: E402
from helpers.persist_float64 import factor_offsets, persistent_or_skip  # noqa: E402
from test_gpu_fullsize_properties import _filled_agent  # noqa: E402

# (mini_epochs, network) -> |persistent - graph| / graph of the last step's gradient norm on the parent commit
PARENT = {(1, "ac"): 1.9598e-06, (1, "cv"): 4.5559e-06, (2, "ac"): 3.5205e-07, (2, "cv"): 6.8709e-07}
UNITS = (1024, 512, 256)


def _lib():
    from seqdex_amd import _abi
    lib = _abi.load_library()
    vp, i32 = C.c_void_p, C.c_int
    lib.sdxpk_input_grams.restype = i32
    lib.sdxpk_input_grams.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    lib.sdxpk_input_grams_reference.restype = i32
    lib.sdxpk_input_grams_reference.argtypes = [vp, i32, vp, i32, vp, vp]
    return lib


_cache = {}


def _device_grams(obs_dim):
    """(obs, cvx0, cvx1 rows, table [8][3][16], reference of (obs, cvx0) [8][2][16], reference of (obs, cvx1)); computed once per width"""
    if obs_dim not in _cache:
        from seqdex_amd.sim import _stream_ptr
        lib, dev = _lib(), torch.device("cuda:0")
        x = [rows(obs_dim, obs_dim), rows(1000 + obs_dim, ST), rows(2000 + obs_dim, ST)]
        d = [torch.from_numpy(v).to(dev) for v in x]
        tab = torch.full((N_MB, 3, 16), float("nan"), device=dev)
        ref = [torch.full((N_MB, 2, 16), float("nan"), device=dev) for _ in range(2)]
        st = _stream_ptr(dev)
        assert lib.sdxpk_input_grams(d[0].data_ptr(), obs_dim, d[1].data_ptr(), d[2].data_ptr(), N_MB, tab.data_ptr(), st) == 0
        for j in range(2):
            assert lib.sdxpk_input_grams_reference(d[0].data_ptr(), obs_dim, d[1 + j].data_ptr(), N_MB, ref[j].data_ptr(), st) == 0
        torch.cuda.synchronize()
        _cache[obs_dim] = (x, tab.cpu().numpy(), ref[0].cpu().numpy(), ref[1].cpu().numpy())
    return _cache[obs_dim]


@pytest.mark.parametrize("obs_dim", [396, 188])
def test_table_equals_the_in_kernel_form_bit_for_bit(obs_dim):
    x, tab, r0, r1 = _device_grams(obs_dim)
    want = np.stack([r0[:, 0], r0[:, 1], r1[:, 1]], axis=1)            # observations, cvx0, cvx1
    asc = np.stack([gram_ascending(v) for v in x], axis=1)
    differ = int((bits(want) != bits(asc)).sum())
    print("obs_dim %d: %d of %d reference entries differ in bits from an ascending float32 sum" % (obs_dim, differ, want.size))
    assert differ > want.size // 2
    np.testing.assert_array_equal(bits(r1[:, 0]), bits(r0[:, 0]))        # the observations' Gram does not depend on the other values of the butterfly
    bad = np.argwhere(bits(tab) != bits(want))
    print("obs_dim %d: %d of %d table entries differ in bits from the reference" % (obs_dim, len(bad), want.size))
    assert len(bad) == 0, "first (minibatch, matrix, entry) %r: table %r reference %r" % (tuple(bad[0]), tab[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("obs_dim", [396, 188])
def test_in_kernel_form_against_float64(obs_dim):
    x, _, r0, r1 = _device_grams(obs_dim)
    for name, v, got in (("observations", x[0], r0[:, 0]), ("cvx0", x[1], r0[:, 1]), ("cvx1", x[2], r1[:, 1])):
        exact, mag = gram_float64(v)
        err = np.abs(got.astype(np.float64) - exact)
        worst = float((err / np.maximum(mag, 1e-300)).max() * 2.0 ** 24)
        print("obs_dim %d %s: max |reference - float64| = %.2f * 2^-24 * sum |a_k b_k| (bound 40)" % (obs_dim, name, worst))
        assert (err <= 40.0 * 2.0 ** -24 * mag).all(), (name, worst)
        diag = got[:, [0, 5, 10, 15]]
        zero_rows = np.abs(v).reshape(N_MB, MB, -1).sum(-1) == 0             # (the all-zero row's own diagonal entry is exactly zero)
        assert (diag[~zero_rows] > 0).all() and (bits(diag[zero_rows]) == 0).all(), name


def _agent(mini_epochs, impl=None):
    """_filled_agent(4, 9) with the mini-epoch count of the case: the same rollout data"""
    import os
    from seqdex_amd.ppo import SdxPPO, make_config
    n, old = 4, os.environ.get("SDXP_UPDATE_IMPL")
    if impl:
        os.environ["SDXP_UPDATE_IMPL"] = impl
    try:
        ag = SdxPPO(n, config=make_config(n, params={"config": {"mini_epochs": mini_epochs}}), seed=9)
    finally:
        if impl:
            if old is None:
                del os.environ["SDXP_UPDATE_IMPL"]
            else:
                os.environ["SDXP_UPDATE_IMPL"] = old
    g = torch.Generator().manual_seed(11)
    for t in range(8):
        obs = torch.randn(n, 396, generator=g).clamp(-5, 5).cuda()
        st = (torch.randn(n, 564, generator=g) * 2).clamp(-5, 5).cuda()
        dones = (torch.rand(n, generator=g) < 0.1).long().cuda()
        eps = torch.randn(n, 23, generator=g).cuda()
        ag.act(t, obs, st, dones, eps)
        ag.store_rewards(t, torch.rand(n, generator=g).cuda(), dones)
    ag.finish_rollout(torch.randn(n, 564, generator=g).cuda(), (torch.rand(n, generator=g) < 0.1).long().cuda())
    torch.cuda.synchronize()
    return ag


def measure_paths(mini_epochs):
    """{network: (persistent norm, graph norm, relative difference)} of the last step of an update of `mini_epochs` mini-epochs"""
    a, b = _agent(mini_epochs), _agent(mini_epochs, impl="graph")
    try:
        persistent_or_skip(a)
        assert b.update_impl() == "graph"
        a.update(); b.update()
        torch.cuda.synchronize()
        ca, cb = a.ctrl(), b.ctrl()
        assert ca.ac_t == cb.ac_t == mini_epochs * N_MB
        return {k: (float(p), float(q), abs(float(p) - float(q)) / float(q)) for k, p, q in (("ac", ca.ac_gnorm, cb.ac_gnorm), ("cv", ca.cv_gnorm, cb.cv_gnorm))}
    finally:
        a.close(); b.close()


def measure_wrong_class():
    """(the central value's gradient norm of minibatch 0 with the Gram of its cvx0 rows, with the Gram of its cvx1 rows, relative move): float64"""
    a = _agent(2)
    try:
        persistent_or_skip(a)
        states = a.t["MB_STATES"].cpu().double().reshape(-1, ST)
        mean, var = a.t["CV_RMS_MEAN"].cpu().double(), a.t["CV_RMS_VAR"].cpu().double()
        cnt = float(a.get_state()["rms_count"])
        a.backward_factors(-1)
        a.backward_factors(0)
        torch.cuda.synchronize()
        F = a.t["FACTORS"].cpu().double()
    finally:
        a.close()
    xo, dyo, ho, dho = factor_offsets()
    # RunningMeanStd in train mode, minibatch by minibatch (k_cv_prenorm): the statistics after the last minibatch are the frozen ones of cvx1
    first = None
    for mb in range(N_MB):
        x = states[MB * mb:MB * mb + MB]
        bm, bv = x.mean(0), x.var(0, unbiased=True)
        delta, tot = bm - mean, cnt + MB
        var = (var * cnt + bv * MB + delta * delta * cnt * MB / tot) / tot
        mean, cnt = mean + delta * MB / tot, tot
        if mb == 0:
            first = ((states[:MB] - mean) / torch.sqrt(var + 1e-5)).clamp(-5, 5)
    cvx1 = ((states[:MB] - mean) / torch.sqrt(var + 1e-5)).clamp(-5, 5)
    cvx0 = F[xo[2, 0]:xo[2, 0] + MB * ST].reshape(MB, ST)
    assert float((cvx0 - first).abs().max()) < 1e-4          # the host restatement of the pre-normalisation is the device's
    n2 = 0.0
    for l in (1, 2):
        x = F[xo[2, l]:xo[2, l] + MB * UNITS[l - 1]].reshape(MB, -1)
        dy = F[dyo[2, l]:dyo[2, l] + MB * UNITS[l]].reshape(MB, -1)
        n2 += float(((dy @ dy.T) * (x @ x.T + 1.0)).sum())
    h = F[ho[2]:ho[2] + MB * UNITS[2]].reshape(MB, -1)
    dv = F[dho:dho + MB * 34].reshape(MB, 34)[:, 33:34]
    n2 += float(((dv @ dv.T) * (h @ h.T + 1.0)).sum())
    dy0 = F[dyo[2, 0]:dyo[2, 0] + MB * UNITS[0]].reshape(MB, -1)
    g0 = dy0 @ dy0.T
    right = float(np.sqrt(n2 + float((g0 * (cvx0 @ cvx0.T + 1.0)).sum())))
    wrong = float(np.sqrt(n2 + float((g0 * (cvx1 @ cvx1.T + 1.0)).sum())))
    return right, wrong, abs(wrong - right) / right


@pytest.mark.parametrize("mini_epochs", [1, 2])
def test_last_steps_gradient_norm_against_the_graph_path(mini_epochs):
    got = measure_paths(mini_epochs)
    for k, (p, q, rel) in got.items():
        print("mini_epochs %d %s: persistent %.9g graph %.9g relative difference %.3e (before the change %.3e, bound %.3e)" % (
            mini_epochs, k, p, q, rel, PARENT[mini_epochs, k], 4.0 * PARENT[mini_epochs, k]))
    for k, (p, q, rel) in got.items():
        assert p > 0.0 and q > 0.0
        assert rel <= 4.0 * PARENT[mini_epochs, k], (mini_epochs, k, p, q, rel)


def test_a_wrong_class_moves_the_norm_far_beyond_the_bound():
    """what makes the test above a test: the other class's Gram moves the central value's norm by more than 100 times its widest bound"""
    right, wrong, move = measure_wrong_class()
    widest = 4.0 * max(PARENT.values())
    print("central value, minibatch 0: norm %.9g, with the cvx1 rows' Gram %.9g, relative move %.3e (widest bound %.3e)" % (right, wrong, move, widest))
    assert right > 0.0 and move > 100.0 * widest, (right, wrong, move)


def test_two_persistent_handles_end_bit_identical():
    n = 16
    a, b = _filled_agent(n, 9), _filled_agent(n, 9)
    try:
        persistent_or_skip(a)
        assert b.update_impl() == "persistent"
        p0 = a.t["AC_PARAMS"].clone()
        a.update(); b.update()
        torch.cuda.synchronize()
        assert a.update_impl() == "persistent" and a.ctrl().ac_t == b.ctrl().ac_t == 5 * (n * 8 // MB) == 160
        for k in ("AC_PARAMS", "CV_PARAMS", "AC_ADAM_M", "AC_ADAM_V", "CV_ADAM_M", "CV_ADAM_V", "MB_MUS", "MB_SIGMAS"):
            np.testing.assert_array_equal(a.t[k].cpu().numpy().view(np.int32), b.t[k].cpu().numpy().view(np.int32), err_msg=k)
        assert float((a.t["AC_PARAMS"] - p0).abs().max()) > 1e-4              # the epoch did something
    finally:
        a.close(); b.close()
