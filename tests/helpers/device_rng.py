"""TEST INFRASTRUCTURE ONLY: numpy restatement of the draws the engine makes for itself from the counter generator sdx_hash
(DESIGN.md section 6), written from that section and the comments at the call sites:

  act noise     h = sdx_hash(seed, counter, env * 64 + column), counter = sdxp_act calls made on the handle so far;
                u1 = (top 24 bits + 1) * (1 / 16777217) in float32 - the divisor rounds to 2^24, so the factor is 2^-24 and u1 lies in
                [2^-24, 1]; u2 = bits 8..31 * 2^-24; eps = sqrt(-2 log u1) * cos(6.28318530718 u2)
  pile choice   sdx_hash(seed, env, step) % K
  insert yaw    half angle 0.785 * (sdx_hash(seed, 0xA11CE, step) & 1): ONE draw per reset event, the plate's quaternion is (0, 0, sin, cos)
  insert slot   sdx_hash(seed ^ 0x5EED, env, step) % min(count, SDX_HARVEST_SLOTS - 1) of the ring of the env's brick type (env % 8)
  search jitter coordinate i = 2 * brick + axis of env e: u = top 24 bits of sdx_hash(seed ^ 0x5EA7, e * 1024 + i, step) * 2^-23 - 1,
                the brick's x / y moves by u * 0.02
  search drop   r = top 24 bits of sdx_hash(seed ^ 0x7A96, e, step) * 2^-23 - 1 places the target brick at (0.25 + 0.2 r, 0.19 + 0.15 r, 0.9)
  tv batch      row r of batch `iter`: dataset row sdx_hash(seed, iter, r) % n of the success set (r < B / 2) or the failure set, component j
                moved by u * 0.05 with u from the top 24 bits of sdx_hash(seed ^ 0x7A11, 4 iter + j, r), then normalised

`step` is the simulator's step counter: post-physics launches since sdx_create (advanced in k_tvalue's finalize branch; no tensor shows it).
Integer draws are exact.  Float draws follow the device's float32 steps one rounding at a time; libm functions are evaluated in float64
and rounded once (the hash itself is tests/helpers/noise_restatement.py's).  Where a draw ends in a multiply-add that the compiler may
contract (the Search jitter and drop: hipcc does, the emulator's g++ build does not) both forms are restated (`contract`, fma32)."""
import numpy as np

from .noise_restatement import _fn, sdx_hash

f32 = np.float32
u64 = np.uint64
NFREE = 72                    # SDX_NFREE
HARVEST_SLOTS = 5001          # SDX_HARVEST_SLOTS
ACT_STREAMS = 64              # stream index of the act noise = env * 64 + column
TAG_SLOT, TAG_JITTER, TAG_DROP, TAG_TV = 0x5EED, 0x5EA7, 0x7A96, 0x7A11
YAW_STREAM = 0xA11CE
U1_SCALE = f32(1.0) / f32(16777217.0)          # the kernel's `1.0f / 16777217.0f`: the divisor is not a float32 number, it rounds to 2^24
U24 = f32(1.0 / 16777216.0)
TWO_PI = f32(6.28318530718)


def _top24(h):
    return ((h >> u64(40)) & u64(0xFFFFFF)).astype(f32)


def uniform_pm1(h):
    """U[-1, 1) on the 2^-23 grid from the top 24 bits: exact in float32"""
    return _top24(h) * f32(2.0 / 16777216.0) - f32(1.0)


def _envs(envs):
    return np.asarray(envs, dtype=u64)


# ---------------------------------------------------------------------------------------------------------------- exploration noise
def act_noise_parts(seed, counter, n_envs, act_dim):
    """(eps, r, c, u1, u2), each [n_envs, act_dim] float32: eps = r * c, r = sqrt(-2 log u1), c = cos(2 pi u2)"""
    env, col = np.meshgrid(np.arange(n_envs, dtype=u64), np.arange(act_dim, dtype=u64), indexing="ij")
    h = sdx_hash(seed, int(counter), env * u64(ACT_STREAMS) + col)
    u1 = (_top24(h) + f32(1.0)) * U1_SCALE
    u2 = ((h >> u64(8)) & u64(0xFFFFFF)).astype(f32) * U24
    r = _fn(np.sqrt, f32(-2.0) * _fn(np.log, u1))
    c = _fn(np.cos, TWO_PI * u2)
    return r * c, r, c, u1, u2


def act_noise(seed, counter, n_envs, act_dim):
    """the eps of sdxp_act call number `counter` (0-based) of a handle created with `seed`, when the caller passes none"""
    return act_noise_parts(seed, counter, n_envs, act_dim)[0]


# ---------------------------------------------------------------------------------------------------------------- reset draws
def pile_choice(seed, envs, step, K):
    return (sdx_hash(seed, _envs(envs), int(step)) % u64(K)).astype(np.int64)


def insert_yaw_half(seed, step):
    """half of the base plate's yaw (float32): 0 or 0.785, the same for every env that resets at `step`"""
    return f32(0.785) * f32(int(sdx_hash(seed, YAW_STREAM, int(step))) & 1)


def insert_slot(seed, envs, step, cnt):
    """`cnt`: ring fill count(s), a number or one per env (the count of ring env % 8); clamped to SDX_HARVEST_SLOTS - 1 as the kernel does"""
    cnt = np.minimum(np.broadcast_to(np.asarray(cnt, dtype=np.int64), np.shape(envs)), HARVEST_SLOTS - 1)
    assert (cnt > 0).all(), "an empty ring draws nothing"
    return (sdx_hash(seed ^ TAG_SLOT, _envs(envs), int(step)) % cnt.astype(u64)).astype(np.int64)


def fma32(a, b, c):
    """a * b + c rounded ONCE to float32 - what the device computes where the compiler contracts a multiply-add.  The product of two
    float32 numbers is exact in float64; so is the sum for the magnitudes these draws have, which is checked (the error term of the
    two-sum is zero)"""
    p, c = np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64), np.asarray(c, f32).astype(np.float64)
    s = p + c
    bb = s - p
    assert not ((p - (s - bb)) + (c - bb)).any(), "a * b + c is not exact in float64 here"
    return s.astype(f32)


def search_jitter_uniform(seed, envs, step):
    """[n, 2 * NFREE] float32 in [-1, 1): the draw of coordinate column % 2 (x, y) of free brick column // 2"""
    e = _envs(envs).reshape(-1, 1)
    i = np.arange(2 * NFREE, dtype=u64).reshape(1, -1)
    return uniform_pm1(sdx_hash(seed ^ TAG_JITTER, e * u64(1024) + i, int(step)))


def search_jitter(seed, envs, step):
    """[n, 2 * NFREE] float32: what is added to x (even columns) and y (odd columns) of free brick column // 2"""
    return search_jitter_uniform(seed, envs, step) * f32(0.02)


def search_jittered(seed, envs, step, lattice, contract):
    """lattice [n, 2 * NFREE] float32 (x, y of the free bricks) after the jitter: fl(lattice + fl(u * 0.02)), or with the multiply-add
    contracted fl(lattice + u * 0.02)"""
    u = search_jitter_uniform(seed, envs, step)
    return fma32(u, f32(0.02), lattice) if contract else np.asarray(lattice, f32) + u * f32(0.02)


def search_drop(seed, envs, step):
    """[n] float32 r in [-1, 1): the ONE draw that moves the target brick in x and y together"""
    return uniform_pm1(sdx_hash(seed ^ TAG_DROP, _envs(envs), int(step)))


def search_drop_pos(seed, envs, step, contract=False):
    """[n, 3] float32: (0.25 + 0.2 r, 0.19 + 0.15 r, 0.9), product and sum rounded one by one or - `contract` - as one multiply-add"""
    r = search_drop(seed, envs, step)
    if contract:
        return np.stack([fma32(r, f32(0.2), f32(0.25)), fma32(r, f32(0.15), f32(0.19)), np.full(r.shape, 0.9, f32)], axis=1)
    return np.stack([f32(0.25) + r * f32(0.2), f32(0.19) + r * f32(0.15), np.full(r.shape, 0.9, f32)], axis=1)


# ---------------------------------------------------------------------------------------------------------------- T-value sampler
def tv_rows(seed, it, n_succ, n_fail, B):
    """dataset row of every batch row: [B] int64, rows [0, B / 2) index the success set, the rest the failure set"""
    r = np.arange(B, dtype=u64)
    n = np.where(np.arange(B) < B // 2, n_succ, n_fail).astype(u64)
    return (sdx_hash(seed, int(it), r) % n).astype(np.int64)


def tv_batch(seed, it, succ, fail, B):
    """[B, 4] float32: the batch number `it` (0-based) of a trainer created with `seed`"""
    succ, fail = np.asarray(succ, f32).reshape(-1, 4), np.asarray(fail, f32).reshape(-1, 4)
    idx = tv_rows(seed, it, succ.shape[0], fail.shape[0], B)
    q = np.where((np.arange(B) < B // 2)[:, None], succ[np.minimum(idx, succ.shape[0] - 1)], fail[np.minimum(idx, fail.shape[0] - 1)])
    r = np.arange(B, dtype=u64)
    v = np.empty((B, 4), f32)
    nn = np.zeros(B, f32)
    for j in range(4):
        u = uniform_pm1(sdx_hash(seed ^ TAG_TV, int(it) * 4 + j, r))
        v[:, j] = q[:, j] + u * f32(0.05)
        nn = nn + v[:, j] * v[:, j]
    return v / _fn(np.sqrt, nn)[:, None]
