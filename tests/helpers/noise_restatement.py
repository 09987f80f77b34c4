"""TEST INFRASTRUCTURE ONLY: numpy restatement of the observation / action noise of DESIGN.md section 18 (include/seqdex.h
sdx_set_noise), written from the definition:

  s        the schedule factor at SDX_T_DR_FRAME[1]: linear min(frame, steps) / steps, constant 0 before steps else 1, none 1
  scaled   gaussian additive: mu, sigma, mu_c, sigma_c x s; gaussian scaling: sigma x s, mu x s + (1 - s); uniform additive: ends x s;
           uniform scaling: end x s + (1 - s) - for the white and the correlated part alike
  operand  corr + white; white = mu + sigma z | lo + (hi - lo) u;  corr = mu_c + sigma_c z | lo_c + (hi_c - lo_c) z  (z normal for both)
  random   h = sdx_hash(seed ^ tag, env * 256 + column // 2, counter); u0 = top 24 bits, u1 = bits 16..39, each (b + 0.5) / 2^24;
           z = sqrt(-2 log u0) * (cos if the column is even else sin)(2 pi u1); u = u0 (even column) or u1 (odd column);
           counter = gravity's draw count (corr) or the step counter (white)
  result   observations clamp(op(obs, operand), +-clip_obs); actions op(clamp(a, +-clip_actions), operand)
  zero     an additive block whose four scaled numbers are zero leaves the tensor as it is

All arithmetic is float32, one rounding per operation, libm functions correctly rounded (float64 evaluation, one rounding)."""
import numpy as np

f32 = np.float32
TAGS = {("observations", "corr"): 0x0B5C, ("observations", "white"): 0x0B57, ("actions", "corr"): 0xAC7C, ("actions", "white"): 0xAC77}
PAIRS = 256
GAUSSIAN, UNIFORM = 1, 2
ADDITIVE, SCALING = 1, 2
_M64 = (1 << 64) - 1


def sdx_hash(seed, a, b):
    """the counter RNG of DESIGN.md section 6 on uint64 arrays `a` and `b` that broadcast together (seed: a Python int; non-negative
    Python ints serve as `a` or `b` too)"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _M64) + np.uint64(0x9E3779B97F4A7C15) * (a + np.uint64(1)) + np.uint64(0xBF58476D1CE4E5B9) * (b + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniforms(h):
    u0 = ((h >> np.uint64(40)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)
    u1 = (((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)
    return u0, u1


def _fn(fn, x):
    return fn(x.astype(np.float64)).astype(f32)


def schedule_factor(attr, frame):
    if attr.schedule == 1:
        return f32(min(int(frame), attr.schedule_steps)) / f32(attr.schedule_steps)
    if attr.schedule == 2:
        return f32(0.0) if frame < attr.schedule_steps else f32(1.0)
    return f32(1.0)


def scaled(attr, s):
    """[white 0, white 1, corr 0, corr 1] as frozen at a non-env randomization"""
    s, one = f32(s), f32(1.0)
    out = []
    for r in (attr.range, attr.range_correlated):
        a, b = f32(r[0]), f32(r[1])
        if attr.operation == SCALING:
            out += [a * s + (one - s), b * s if attr.distribution == GAUSSIAN else b * s + (one - s)]
        else:
            out += [a * s, b * s]
    return out


def is_zero(attr, frame):
    return attr.operation == ADDITIVE and all(v == 0 for v in scaled(attr, schedule_factor(attr, frame)))


def _ulp(x):
    return np.spacing(np.abs(x).astype(f32)).astype(np.float64)


def parts(attr, seed, tensor, n_envs, width, draw, step, frame):
    """(corr, white, bound_corr, bound_white): [n_envs, width] float32 parts of the operand and an absolute bound on what a device draw
    may differ by: 2 ulp of a gaussian draw sigma * z (the sampler's bound) plus one rounding where a non-zero
    centre is added, 0 for a uniform draw and for a part whose spread is zero (c + 0 * z is exact)"""
    p = scaled(attr, schedule_factor(attr, frame))
    env, col = np.meshgrid(np.arange(n_envs, dtype=np.uint64), np.arange(width, dtype=np.uint64), indexing="ij")
    stream = env * np.uint64(PAIRS) + (col >> np.uint64(1))
    odd = (col & np.uint64(1)).astype(bool)

    def normal(h):
        u0, u1 = uniforms(h)
        r, th = _fn(np.sqrt, f32(-2.0) * _fn(np.log, u0)), f32(6.28318530718) * u1
        return r * np.where(odd, _fn(np.sin, th), _fn(np.cos, th))

    hc = sdx_hash(seed ^ TAGS[(tensor, "corr")], stream, int(draw))
    hw = sdx_hash(seed ^ TAGS[(tensor, "white")], stream, int(step))
    def gaussian_part(centre, spread, z):
        # the sampler's bound is 2 ulp of a draw sigma * z around a centre of zero (every gaussian block the engine ships); a centre that
        # is not zero adds one rounding (1 ulp of the sum for an input that moved), and a zero spread makes the part exact (c + 0 * z)
        term = (spread * z).astype(f32)
        part = (centre + term).astype(f32)
        if spread == 0:
            return part, np.zeros(part.shape)
        return part, 2.0 * _ulp(term) + (_ulp(part) if centre != 0 else 0.0)

    if attr.distribution == GAUSSIAN:
        corr, bc = gaussian_part(p[2], p[3], normal(hc))
        white, bw = gaussian_part(p[0], p[1], normal(hw))
    else:
        corr, bc = gaussian_part(p[2], p[3] - p[2], normal(hc))
        u0, u1 = uniforms(hw)
        white = (p[0] + (p[1] - p[0]) * np.where(odd, u1, u0)).astype(f32)       # exact: products and sums of float32 numbers
        bw = np.zeros(white.shape)
    return corr, white, bc, bw


def operand(attr, seed, tensor, n_envs, width, draw, step, frame):
    """(operand [n_envs, width] float32, absolute bound float64).  The bound: the two draws' bounds, plus - when either is non-zero - one
    ulp of the sum, because a sum of inputs that moved by d can round to a neighbour one ulp further than d"""
    corr, white, bc, bw = parts(attr, seed, tensor, n_envs, width, draw, step, frame)
    o = (corr + white).astype(f32)
    b = bc + bw
    return o, b + np.where(b > 0, _ulp(o), 0.0)


def apply(attr, x, o, bound, clip, tensor, frame):
    """(expected tensor, absolute tolerance) for input rows x (the clean observation, or the caller's actions) and the operand above.
    Tolerance: the operand's bound carried through the operation (additive: as it is; scaling: x |x|), plus one ulp of the result for the
    operation's own rounding of a moved input - except where that operation is exact whatever the operand (0 + o = o)."""
    x = np.asarray(x, f32)
    if tensor == "actions":
        x = np.minimum(f32(clip), np.maximum(f32(-clip), x))
    if is_zero(attr, frame):
        y = x if tensor == "actions" else np.minimum(f32(clip), np.maximum(f32(-clip), x))
        return y, np.zeros(x.shape)
    if attr.operation == ADDITIVE:
        y = (x + o).astype(f32)
        tol = bound + np.where((x == 0) | (bound == 0), 0.0, _ulp(y))
    else:
        y = (x * o).astype(f32)
        tol = np.abs(x).astype(np.float64) * bound + np.where(bound == 0, 0.0, _ulp(y))
    if tensor == "observations":
        y = np.minimum(f32(clip), np.maximum(f32(-clip), y))
    return y, tol
