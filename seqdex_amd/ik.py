"""The parameters and the result of SdxSim.solve_ik (include/seqdex.h sdx_solve_ik): arm and fingertip inverse
kinematics in one launch.  No kernel and no tensor expression of its own."""
import collections

TASKS = ("base", "ff", "mf", "rf", "th")      # bit t of sdx_ik_attr.task_mask and of the converged mask

# what SdxSim.solve_ik returns: q [N, 23] the solution, err [N, 6] = |position error|, |rotation error| of the hand base and |position error| of
# the four tips at q (+0.0 for a task that was not selected), converged bool [N, 5] one column per task of TASKS, iters int32 [N, 5] the
# steps each task took
IkSolution = collections.namedtuple("IkSolution", ["q", "err", "converged", "iters"])


class IkParams(collections.namedtuple("IkParams", ["tasks", "max_iters", "damping_arm", "damping_finger", "max_step", "pos_tol", "rot_tol",
                                                   "tip_offset"])):
    """the parameters of SdxSim.solve_ik (sdx_ik_attr).  tasks: names out of TASKS; tip_offset: None (zeros), 3 numbers (every finger) or 4 x 3:
    the controlled point of each fingertip in the frame of its fingertip link.  damping_arm 0.05 is control_ik's; damping_finger 0.01
    because a finger's lever arms are centimetres; a tolerance of 0 never stops early."""
    __slots__ = ()

    def __new__(cls, tasks=TASKS, max_iters=32, damping_arm=0.05, damping_finger=0.01, max_step=0.2, pos_tol=1e-4, rot_tol=1e-3,
                tip_offset=None):
        tasks = (tasks,) if isinstance(tasks, str) else tuple(tasks)
        for t in tasks:
            if t not in TASKS:
                raise ValueError("IkParams: tasks takes names out of %s, got %r" % (TASKS, t))
        if tip_offset is None:
            off = ((0.0, 0.0, 0.0),) * 4
        else:
            rows = list(tip_offset)
            if len(rows) == 3 and all(isinstance(v, (int, float)) for v in rows):
                rows = [rows] * 4
            if len(rows) != 4 or any(isinstance(r, (int, float)) or len(r) != 3 for r in rows):
                raise ValueError("IkParams: tip_offset takes 3 numbers or 4 rows of 3, got %r" % (tip_offset,))
            off = tuple(tuple(float(v) for v in r) for r in rows)
        return super().__new__(cls, tasks, int(max_iters), float(damping_arm), float(damping_finger), float(max_step), float(pos_tol),
                               float(rot_tol), off)

    @property
    def task_mask(self):
        return sum(1 << TASKS.index(t) for t in set(self.tasks))

    def to_attr(self):
        """the _abi.IkAttr of these parameters"""
        from . import _abi
        a = _abi.IkAttr()
        a.task_mask, a.max_iters = self.task_mask, self.max_iters
        a.damping_arm, a.damping_finger, a.max_step = self.damping_arm, self.damping_finger, self.max_step
        a.pos_tol, a.rot_tol = self.pos_tol, self.rot_tol
        for f in range(4):
            a.tip_offset[f][:] = self.tip_offset[f]
        return a
