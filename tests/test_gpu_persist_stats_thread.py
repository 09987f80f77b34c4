"""-m gpu: the statistics / learning-rate thread of the persistent update kernel (dY1 shadow; csrc/sdxp_persist_tails.h: stats_lr_once).  One thread
per CU adds the minibatch's per-sample loss statistics (S.stat), folds the six means into the epoch's running sums, keeps last_kl and applies the
legacy adaptive learning-rate rule; every wave of the CU waits for it at the shadow's closing barrier.  stats_lr_once requests the 24 statistics,
the six running sums and ac_lr in one LDS round trip where the serial loop made twelve dependent ones, and keeps the arithmetic:

    t_j = ((((0 + stat[0][j]) + stat[1][j]) + stat[2][j]) + stat[3][j]),   sum_j = fma(t_j, 1/4, sum_j),   kl = t_kl * 1/4
    kl > 2 threshold: lr = max(lr / 1.5, 1e-6)        kl < threshold / 2: lr = min(lr * 1.5, 1e-2)                    (adaptive only)

The test entry sdxpk_stats_thread_check (csrc/sdxp_persist_checks.hip, built with the epoch kernel's flags) runs stats_lr_once beside the serial
loop, kept there verbatim, one workgroup per case.  new == serial loop == a numpy float32 restatement, bit for bit, in the six sums, last_kl and
ac_lr.  (t * 1/4 is exact, so the fma and a product followed by an add give the same bits; the division is IEEE in both.)

Statistics and running sums as in test_gpu_persist_ordered_sum.py: 13 random significant bits at exponents spread over 2^-12 .. 2^12, mixed signs.
The KL column, the threshold and ac_lr of the first cases are set so that - asserted on the host first - the cases reach: kl above twice the
threshold, below half of it, between the two, the adaptive flag off (with a kl that would move the rate), ac_lr at its floor 1e-6 and asked to
fall, ac_lr at its cap 1e-2 and asked to rise."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MB, CASES = 4, 40
KL = 4                                   # STAT_KL (csrc/sdxp_persist_lds.h); columns 1..6 are read
f32 = np.float32


def _values(r, shape):
    m = r.integers(1 << 12, 1 << 13, size=shape).astype(np.float64)
    return (m * 2.0 ** r.integers(-24, 1, size=shape) * r.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def _kl(stat):
    t = f32(0.0)
    for s in range(MB):
        t = f32(t + stat[s][KL])
    return f32(t * f32(0.25))


def _inputs():
    """in [CASES][40]: stat [MB][8], six running sums, ac_lr, kl_threshold; adaptive [CASES]; kind [CASES]"""
    r = np.random.default_rng(31)
    x = _values(r, (CASES, 40))
    x[:, 38] = (1e-6 + r.random(CASES) * (1e-2 - 1e-6)).astype(np.float32)       # ac_lr inside its range
    x[:, 39] = np.abs(x[:, 39])                                                 # thresholds are positive
    adaptive = np.ones(CASES, np.int32)
    kind = ["random"] * CASES
    for c, k in enumerate(["above", "below", "between", "off", "floor", "cap"] * 4):
        stat = x[c, :32].reshape(MB, 8)
        stat[:, KL] = np.abs(stat[:, KL])                                       # a positive kl, as the loss phase produces
        kl = _kl(stat)
        x[c, 39] = {"above": kl / f32(4), "below": kl * f32(4), "between": kl, "off": kl / f32(4), "floor": kl / f32(4), "cap": kl * f32(4)}[k]
        if k == "off":
            adaptive[c] = 0
        if k == "floor":
            x[c, 38] = f32(1e-6) if c < 12 else f32(1.2e-6)                      # at the floor / one step above it: lr / 1.5 falls below
        if k == "cap":
            x[c, 38] = f32(1e-2) if c < 12 else f32(8e-3)
        kind[c] = k
    return x, adaptive, kind


def _restate(x, adaptive):
    """the thread's arithmetic in numpy float32 -> [8]: six sums, last_kl, ac_lr; and which branches of the rule fired"""
    stat = x[:32].reshape(MB, 8)
    out = np.zeros(8, np.float32)
    for j in range(6):
        t = f32(0.0)
        for s in range(MB):
            t = f32(t + stat[s][1 + j])
        out[j] = f32(x[32 + j] + f32(t * f32(0.25)))                            # == fma(t, 1/4, sum): the product is exact
    kl, lr, thr = _kl(stat), f32(x[38]), f32(x[39])
    fell = rose = False
    if adaptive:
        if kl > f32(2.0) * thr:
            lr, fell = max(f32(lr / f32(1.5)), f32(1e-6)), True
        if kl < f32(0.5) * thr:
            lr, rose = min(f32(lr * f32(1.5)), f32(1e-2)), True
    out[6], out[7] = kl, lr
    return out, fell, rose


def test_one_round_trip_keeps_sums_kl_and_learning_rate():
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib, dev = _abi.load_library(), torch.device("cuda:0")
    lib.sdxpk_stats_thread_check.restype = C.c_int
    lib.sdxpk_stats_thread_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    x, adaptive, kind = _inputs()
    want = np.zeros((CASES, 8), np.float32)
    reached = {k: 0 for k in ("above", "below", "between", "off", "floor", "cap")}
    for c in range(CASES):
        want[c], fell, rose = _restate(x[c], adaptive[c])
        lr0 = x[c, 38]
        if kind[c] == "above":
            reached["above"] += fell and not rose and want[c, 7] < lr0
        elif kind[c] == "below":
            reached["below"] += rose and not fell and want[c, 7] > lr0
        elif kind[c] == "between":
            reached["between"] += adaptive[c] == 1 and not fell and not rose and want[c, 7] == lr0
        elif kind[c] == "off":
            reached["off"] += adaptive[c] == 0 and want[c, 6] > f32(2.0) * x[c, 39] and want[c, 7] == lr0
        elif kind[c] == "floor":
            reached["floor"] += fell and want[c, 7] == f32(1e-6)
        elif kind[c] == "cap":
            reached["cap"] += rose and want[c, 7] == f32(1e-2)
    print("cases that reach each branch of the rule: %s; free cases: %d" % (reached, kind.count("random")))
    assert all(v >= 4 for v in reached.values()), reached
    d_x, d_a = torch.from_numpy(x).to(dev), torch.from_numpy(adaptive).to(dev)
    out = torch.full((CASES, 2, 8), float("nan"), device=dev)
    assert lib.sdxpk_stats_thread_check(d_x.data_ptr(), d_a.data_ptr(), CASES, out.data_ptr(), _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    serial, new = np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1])
    assert not np.isnan(serial).any() and not np.isnan(new).any()
    print("serial loop against the host: %d, stats_lr_once against the serial loop: %d of %d values differ in bits" % (
        int((serial.view(np.int32) != want.view(np.int32)).sum()), int((new.view(np.int32) != serial.view(np.int32)).sum()), want.size))
    np.testing.assert_array_equal(serial.view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(new.view(np.int32), serial.view(np.int32))
