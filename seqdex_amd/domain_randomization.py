"""Domain randomization: `cfg["task"]["randomization_params"]` (the reference's schema, BT:229-420) -> sdx_dr_desc and the two
sdx_noise_attr of include/seqdex.h.

The sampling itself runs on the device (sdx_set_randomization, sdx_set_noise, sdx_step); this module only parses and validates the YAML
block and reports what it does with every entry: `parse` the physics descriptor, `parse_noise` the `observations` / `actions` blocks
that BaseTask.step applies (BT:131-132,149-150).  The rules are written out in DESIGN.md section 18."""
import ctypes as C
import math
import warnings

from ._abi import NoiseAttr

DISTRIBUTIONS = {"gaussian": 1, "uniform": 2, "loguniform": 3}
OPERATIONS = {"additive": 1, "scaling": 2}
SCHEDULES = {None: 0, "linear": 1, "constant": 2}
ATTR_KEYS = {"range", "operation", "distribution", "schedule", "schedule_steps", "num_buckets"}

# YAML path -> sdx_dr_desc field
SUPPORTED = {
    ("sim_params", "gravity"): "gravity",
    ("actor_params", "hand", "dof_properties", "stiffness"): "dof_stiffness",
    ("actor_params", "hand", "dof_properties", "damping"): "dof_damping",
    ("actor_params", "hand", "dof_properties", "lower"): "dof_lower",
    ("actor_params", "hand", "dof_properties", "upper"): "dof_upper",
    ("actor_params", "hand", "rigid_body_properties", "mass"): "link_mass",
    ("actor_params", "hand", "rigid_shape_properties", "friction"): "link_friction",
    ("actor_params", "lego", "rigid_body_properties", "mass"): "brick_mass",
    ("actor_params", "lego", "rigid_shape_properties", "friction"): "brick_friction",
}
# not part of the physics descriptor `parse` builds: `parse_noise` reads these two blocks (SdxSim.set_noise applies them)
_NOOP_TOP = {"observations": "observation noise: not a physics parameter; parse_noise() reads it and SdxSim.set_noise() applies it",
             "actions": "action noise: not a physics parameter; parse_noise() reads it and SdxSim.set_noise() applies it"}
NOISE_KEYS = {"range", "range_correlated", "operation", "distribution", "schedule", "schedule_steps"}
NOISE_DISTRIBUTIONS = {"gaussian": 1, "uniform": 2}
_NOOP_PROP = {"tendon_properties": "the hand has no tendons", "color": "visual only"}
_UNSUPPORTED = {"scale": "per-env brick scale needs per-env collision geometry (out of scope)"}
_ACTOR_PROPS = {"hand": {"dof_properties", "rigid_body_properties", "rigid_shape_properties"},
                "lego": {"rigid_body_properties", "rigid_shape_properties"}}
_PROP_ATTRS = {"dof_properties": {"stiffness", "damping", "lower", "upper"}, "rigid_body_properties": {"mass"},
               "rigid_shape_properties": {"friction"}}
_warned = set()


class DrAttr(C.Structure):
    """sdx_dr_attr"""
    _fields_ = [("distribution", C.c_int32), ("operation", C.c_int32), ("schedule", C.c_int32), ("schedule_steps", C.c_int32),
                ("num_buckets", C.c_int32), ("range", C.c_float * 2)]


FIELDS = ("gravity", "dof_stiffness", "dof_damping", "dof_lower", "dof_upper", "link_mass", "link_friction", "brick_mass", "brick_friction")


class DrDesc(C.Structure):
    """sdx_dr_desc"""
    _fields_ = [("frequency", C.c_int32)] + [(f, DrAttr) for f in FIELDS]


def _attr(path, spec):
    name = ".".join(path)
    if not isinstance(spec, dict):
        raise ValueError("randomization_params.%s: expected a mapping, got %r" % (name, spec))
    extra = set(spec) - ATTR_KEYS
    if extra:
        raise ValueError("randomization_params.%s: unknown key(s) %s" % (name, sorted(extra)))
    a = DrAttr()
    for key, table in (("distribution", DISTRIBUTIONS), ("operation", OPERATIONS), ("schedule", SCHEDULES)):
        if spec.get(key) not in table:
            raise ValueError("randomization_params.%s.%s: unknown %s %r" % (name, key, key, spec.get(key)))
        setattr(a, key, table[spec.get(key)])
    if a.schedule:
        if int(spec.get("schedule_steps", 0)) <= 0:
            raise ValueError("randomization_params.%s.schedule_steps: a schedule needs schedule_steps > 0" % name)
        a.schedule_steps = int(spec["schedule_steps"])
    a.num_buckets = int(spec.get("num_buckets", 0))
    r = spec.get("range")
    if not isinstance(r, (list, tuple)) or len(r) != 2:
        raise ValueError("randomization_params.%s.range: expected [lo, hi] (or [mu, sigma])" % name)
    a.range[0], a.range[1] = float(r[0]), float(r[1])
    if a.distribution == DISTRIBUTIONS["loguniform"] and not (a.range[0] > 0 and a.range[1] > 0):
        raise ValueError("randomization_params.%s.range: loguniform needs positive ends" % name)
    if a.distribution == DISTRIBUTIONS["gaussian"] and a.range[1] < 0:
        raise ValueError("randomization_params.%s.range: a gaussian's sigma must be >= 0" % name)
    if a.distribution != DISTRIBUTIONS["gaussian"] and a.range[0] > a.range[1]:
        raise ValueError("randomization_params.%s.range: lo > hi" % name)
    if a.num_buckets < 0 or (a.num_buckets > 0 and a.distribution == DISTRIBUTIONS["loguniform"]):
        raise ValueError("randomization_params.%s.num_buckets: buckets apply to uniform and gaussian, >= 0" % name)
    return a


def parse(params):
    """randomization_params -> (DrDesc, report).  report = {"randomized": [paths], "noop": {path: why}, "unsupported": {path: why}}.
    Unknown actors, properties, attributes, distributions, operations and schedules raise ValueError naming the key."""
    if not params:
        raise ValueError("task.randomize is True but task.randomization_params is empty: nothing to randomize")
    if not isinstance(params, dict):
        raise ValueError("task.randomization_params: expected a mapping")
    d = DrDesc()
    d.frequency = int(params.get("frequency", 1))          # BT:231
    if d.frequency < 1:
        raise ValueError("randomization_params.frequency: must be >= 1")
    rep = {"randomized": [], "noop": {}, "unsupported": {}}
    for top, v in params.items():
        if top == "frequency":
            continue
        if top in _NOOP_TOP:
            rep["noop"][top] = _NOOP_TOP[top]
        elif top == "sim_params":
            for attr, spec in (v or {}).items():
                if (top, attr) not in SUPPORTED:
                    raise ValueError("randomization_params.sim_params.%s: unknown simulation parameter" % attr)
                setattr(d, SUPPORTED[(top, attr)], _attr((top, attr), spec))
                rep["randomized"].append("sim_params." + attr)
        elif top == "actor_params":
            for actor, props in (v or {}).items():
                if actor not in _ACTOR_PROPS:
                    raise ValueError("randomization_params.actor_params.%s: unknown actor (hand, lego)" % actor)
                for prop, attrs in (props or {}).items():
                    path = "actor_params.%s.%s" % (actor, prop)
                    if prop in _NOOP_PROP:
                        rep["noop"][path] = _NOOP_PROP[prop]
                        continue
                    if prop in _UNSUPPORTED and actor == "lego":
                        rep["unsupported"][path] = _UNSUPPORTED[prop]
                        if path not in _warned:   # once per process
                            _warned.add(path)
                            warnings.warn("seqdex_amd: randomization_params.%s is not supported and is ignored: %s"
                                          % (path, _UNSUPPORTED[prop]), RuntimeWarning, stacklevel=2)
                        continue
                    if prop not in _ACTOR_PROPS[actor]:
                        raise ValueError("randomization_params.%s: unknown property" % path)
                    for attr, spec in (attrs or {}).items():
                        if attr not in _PROP_ATTRS[prop]:
                            raise ValueError("randomization_params.%s.%s: unknown attribute" % (path, attr))
                        key = ("actor_params", actor, prop, attr)
                        setattr(d, SUPPORTED[key], _attr(key, spec))
                        rep["randomized"].append("%s.%s" % (path, attr))
        else:
            raise ValueError("randomization_params.%s: unknown key" % top)
    return d, rep


def identity_desc(frequency=1):
    """a desc with no attribute randomized: turns the per-env physics path on without sampling (caller-supplied rows, tests)"""
    d = DrDesc()
    d.frequency = frequency
    return d


def _pair(name, key, v):
    if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in v):
        raise ValueError("randomization_params.%s.%s: expected two numbers ([mu, sigma] or [lo, hi]), got %r" % (name, key, v))
    if not all(math.isfinite(float(x)) for x in v):
        raise ValueError("randomization_params.%s.%s: not finite: %r" % (name, key, v))
    return float(v[0]), float(v[1])


def _noise_attr(name, spec):
    if not isinstance(spec, dict):
        raise ValueError("randomization_params.%s: expected a mapping, got %r" % (name, spec))
    extra = set(spec) - NOISE_KEYS
    if extra:
        raise ValueError("randomization_params.%s: unknown key(s) %s" % (name, sorted(extra)))
    a = NoiseAttr()
    for key, table in (("distribution", NOISE_DISTRIBUTIONS), ("operation", OPERATIONS), ("schedule", SCHEDULES)):
        if spec.get(key) not in table:
            raise ValueError("randomization_params.%s.%s: unknown %s %r" % (name, key, key, spec.get(key)))
        setattr(a, key, table[spec.get(key)])
    if a.schedule:
        steps = spec.get("schedule_steps")
        if not isinstance(steps, int) or isinstance(steps, bool) or steps <= 0:
            raise ValueError("randomization_params.%s.schedule_steps: a schedule needs schedule_steps > 0, got %r" % (name, steps))
        a.schedule_steps = steps
    if "range" not in spec:
        raise ValueError("randomization_params.%s.range: missing" % name)
    for key in ("range", "range_correlated"):
        lo, hi = _pair(name, key, spec.get(key, [0.0, 0.0]))          # BT:277,307: range_correlated defaults to [0, 0]
        if a.distribution == NOISE_DISTRIBUTIONS["gaussian"] and hi < 0:
            raise ValueError("randomization_params.%s.%s: a gaussian's sigma must be >= 0" % (name, key))
        if a.distribution == NOISE_DISTRIBUTIONS["uniform"] and lo > hi:
            raise ValueError("randomization_params.%s.%s: lo > hi" % (name, key))
        getattr(a, key)[0], getattr(a, key)[1] = lo, hi
    return a


def parse_noise(params):
    """randomization_params -> (observations NoiseAttr or None, actions NoiseAttr or None, report).  Only the `observations` and
    `actions` blocks are read (the rest is `parse`'s); report = {block: its values as applied} for the blocks present.  Unknown keys,
    distributions, operations and schedules, a schedule without schedule_steps and a bad range / range_correlated raise ValueError
    naming the key."""
    if params is not None and not isinstance(params, dict):
        raise ValueError("task.randomization_params: expected a mapping")
    out, rep = [], {}
    for name in ("observations", "actions"):
        spec = (params or {}).get(name)
        if spec is None:
            out.append(None)
            continue
        a = _noise_attr(name, spec)
        out.append(a)
        rep[name] = {"distribution": spec["distribution"], "operation": spec["operation"], "schedule": spec.get("schedule"),
                     "schedule_steps": int(a.schedule_steps), "range": [float(v) for v in spec["range"]],
                     "range_correlated": [float(v) for v in spec.get("range_correlated", [0.0, 0.0])]}
    return out[0], out[1], rep
