"""Shared by tests/test_chain_line_cpu.py and tests/test_chain_line_gpu.py: the arms and cases that hold naf_chain_line_track
(csrc/chain_env.hip) against the float64 rule of environment/line_moves.py (track_line, line_record, line_verdict), built with the
twin alone; a float32 numpy restatement of the tracker from the existing restatements of its updates (chain_ik_common.ik_step32,
chain_ik_pose_common.ik_pose_step32 / walk32) that stands in for the device in the CPU rehearsal; and the checks both suites apply
to what a tracker — that restatement, or the kernel — returned."""
import functools

import numpy as np

import chain_ik_common as IK
import chain_ik_pose_common as P
import chain_rollout_common as C

from robotic_manipulator_rloa_amd.environment import line_moves as LM
from robotic_manipulator_rloa_amd.environment.line_moves import HOLD_AXIS, HOLD_FULL, HOLD_POSITION

ORAD = IK.ORAD
TOLERANCE = float(np.float32(1e-3))
ORIENTATION_TOLERANCE = float(np.float32(1e-3))
CAP = C.CAP                        # the project's band rule: at most 1 % of a case inside a band
ARMS = ["iiwa_like7", "long12", "slider4"]
COUNTS = [(1, 1, 1), (5, 16, 2), (65, 8, 4), (4, 63, 1)]      # (N, W, U): one lane and one waypoint, a partial wave, a second wave
                                                             # of one lane, the longest polyline
MODES = [HOLD_FULL, HOLD_AXIS, HOLD_POSITION]
CASES = [(name, N, W, U, mode) for name in ARMS for N, W, U in COUNTS for mode in MODES]
TOOL_AXIS, TOOL_NORMAL = P.TOOL_AXIS, P.TOOL_NORMAL
SHORT, LONG = 0.05, 0.6            # displacement lengths in reaches: a line that is tracked, one that runs into limits or reach

# The bounds. test_chain_line_cpu.test_rehearsal measures, over every case above, with the float32 restatement (track32) in the
# kernel's place: the largest max-norm deviation of a single restated update from the twin's step (ik_step / ik_pose_step) at the same
# recorded pose, teacher-forced over all W U updates — the updates §24's rule leaves out (the twin's pose has quaternion w < 1e-3,
# full, or |t x d| < 1e-2 with t . d < 0, axis) are none in any case: the held orientation is the start's own — and the largest
# deviation of the four record floats evaluated in float32 at the restatement's nodes from line_record in float64 at the same nodes:
#     step     : iiwa_like7 5.57e-6, long12 2.35e-5, slider4 4.25e-6 (largest at long12, 65 x 8 x 4, axis)
#     residual : iiwa_like7 3.42e-7, long12 2.51e-7, slider4 2.10e-7
#     angle    : iiwa_like7 3.92e-7, long12 4.98e-7, slider4 3.23e-7
#     mid-leg  : iiwa_like7 2.69e-7, long12 2.20e-7, slider4 2.01e-7
#     [2], the joint step, is the float32 difference of two float32 values: it is held bit for bit, not within a bound
#     ->  STEP_DEVIATION = 2.5e-5 rad, RESIDUAL_DEVIATION = 4e-7 m, ANGLE_DEVIATION = 6e-7 rad, MID_DEVIATION = 3.5e-7 m, rounded up
# slider4 holds no orientation along a drawn line (four joints, two of them prismatic): all its full and axis queries are 'lost', as
# they should be, and only its position cases hold both verdicts; every other case of 64 or more queries holds both.
# The GPU bounds are 8 x these, for the reason chain_ik_common gives for its STEP_BOUND: a second float32 evaluation of the same
# expressions differs from the first by the same mechanism and no more than a small multiple of it. They are taken from the
# restatement, never from the kernel. No query of any case has a tracked waypoint above a quarter of a tolerance or a first lost
# waypoint below four times one (the pool filter of build_case keeps none), so every band share is 0 of N.
STEP_DEVIATION = 2.5e-5
RESIDUAL_DEVIATION = 4e-7
ANGLE_DEVIATION = 6e-7
MID_DEVIATION = 3.5e-7
STEP_BOUND = 8 * STEP_DEVIATION
RESIDUAL_BOUND = 8 * RESIDUAL_DEVIATION
ANGLE_BOUND = 8 * ANGLE_DEVIATION
MID_BOUND = 8 * MID_DEVIATION


def f32(x):
    return C.f32(x)


def constants(model):
    """the updates' constants as device and twin are given them (float32 values): line_constants'"""
    return LM.line_constants(model)


# ---- the float32 restatement ----------------------------------------------------------------------------------------------------
def goal32(model, q_start, mode):
    """(p0[N, 3], goal) in float32 from the restated walk at q_start: R_ee row-major [N, 9] (full), R_ee tool_axis [N, 3] (axis)"""
    ee, R, _, _ = P.walk32(model, q_start)
    if mode == HOLD_FULL:
        return ee, R.reshape(R.shape[:-2] + (9,))
    return ee, (R @ TOOL_AXIS.astype(np.float32) if mode == HOLD_AXIS else None)


def step32(model, q, g, mode, goal, c):
    if mode == HOLD_POSITION:
        return IK.ik_step32(model, q, g, c["lam2"], c["e_max"], c["dq_max"])
    return P.ik_pose_step32(model, q, g, mode, goal, c)


def record32(model, prev, q, p0, disp, i, W, mode, goal):
    """waypoint i's four floats in float32, as the kernel forms them"""
    f = np.float32
    ee, R, _, _ = P.walk32(model, q)
    d = (p0 + (f(i) / f(W)) * disp) - ee
    residual = np.sqrt(np.sum(d * d, axis=-1))
    if mode == HOLD_POSITION:
        angle = np.zeros(residual.shape, f)
    else:
        w = P.orientation_error32(R, mode, goal)
        angle = np.sqrt(np.sum(w * w, axis=-1))
    mid, _, _, _ = P.walk32(model, (q + prev) * f(0.5))
    h = mid - (p0 + ((f(i) - f(0.5)) / f(W)) * disp)
    out = np.stack([residual, angle, np.max(np.abs(q - prev), axis=-1), np.sqrt(np.sum(h * h, axis=-1))], axis=-1)
    assert out.dtype == f
    return out


def track32(case):
    """What naf_chain_line_track returns, by the restatement: dict of nodes[N, W + 1, A], track[N, W, 4], iters[W U + 1, N, A]"""
    model, c, W, U, mode = case.model, constants(case.model), case.W, case.U, case.mode
    f = np.float32
    q, disp = case.q_start.astype(f), case.disp.astype(f)
    p0, goal = goal32(model, q, mode)
    nodes, iters, track = [q], [q], []
    for i in range(1, W + 1):
        g, prev = p0 + (f(i) / f(W)) * disp, q
        for _ in range(U):
            q = step32(model, q, g, mode, goal, c)
            iters.append(q)
        track.append(record32(model, prev, q, p0, disp, i, W, mode, goal))
        nodes.append(q)
    return dict(nodes=np.stack(nodes, axis=1), track=np.stack(track, axis=1), iters=np.stack(iters))


# ---- cases ------------------------------------------------------------------------------------------------------------------------
class LineCase:
    """N lines of one arm, all float32 values held as float64: q_start[N, A], disp[N, 3]; W waypoints of U updates, the hold mode"""

    def __init__(self, name, N, W, U, mode, q_start, disp):
        self.name, self.N, self.W, self.U, self.mode = name, N, W, U, mode
        self.model, self.twin = IK.arm(name)
        self.q_start, self.disp = q_start, disp

    @functools.lru_cache(maxsize=None)
    def twin_solution(self):
        """(nodes[N, W + 1, A], track[N, W, 4], iters[W U + 1, N, A]) of the float64 rule: computed once, shared, never changed"""
        out = LM.track_line(self.twin, self.q_start, self.disp, self.mode, self.W, self.U, constants(self.model), TOOL_AXIS, TOOL_NORMAL,
                            record=True)
        for a in out:
            a.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def held(self):
        """(p0[N, 3], goal) of the twin at q_start"""
        R0, p0 = self.twin.end_effector_frame(self.q_start)
        return p0, (R0 if self.mode == HOLD_FULL else R0 @ TOOL_AXIS)

    def sub(self, rows):
        return LineCase(self.name, len(rows), self.W, self.U, self.mode, self.q_start[rows], self.disp[rows])


def merits(track):
    """[N, W]: max(residual / tolerance, angle / orientation_tolerance) per waypoint"""
    return np.maximum(track[:, :, 0] / TOLERANCE, track[:, :, 1] / ORIENTATION_TOLERANCE)


def verdict(track):
    return LM.line_verdict(track, track.dtype.type(TOLERANCE), track.dtype.type(ORIENTATION_TOLERANCE))[0]


def sure(track):
    """[N] bool: the verdict of these records has room to spare — every waypoint of the tracked prefix is within a quarter of both
    tolerances and the first lost one, where there is one, misses one of them by a factor of four"""
    m = merits(np.asarray(track, np.float64))
    K = verdict(np.asarray(track, np.float64))
    W = m.shape[1]
    inside = np.arange(W)[None, :] < K[:, None]
    lost = np.take_along_axis(m, np.minimum(K, W - 1)[:, None], axis=1)[:, 0]
    return (np.where(inside, m, 0.0).max(axis=1) <= 0.25) & ((K == W) | (lost > 4.0))


@functools.lru_cache(maxsize=None)
def build_case(name, N, W, U, mode, seed=0):
    """Start poses free and inside the limits; displacements in drawn directions, in turn SHORT and LONG reaches long. A pool is
    tracked by the float64 rule and a query is kept when its verdict has room to spare (sure): no kept query has a tracked waypoint
    above a quarter of a tolerance or a first lost waypoint below four times one. Where both verdicts are left in the pool, even
    queries are taken from the fully tracked and odd ones from the lost."""
    model, twin = IK.arm(name)
    rng = np.random.default_rng(11000 + 131 * N + 7 * W + U + 1000 * mode + seed)
    pool = 4 * N + 32
    starts = IK.free_poses(model, twin, rng, pool)
    d = rng.normal(size=(pool, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    disp = f32(d * np.where(np.arange(pool) % 2 == 0, SHORT, LONG)[:, None] * model.reach)
    trial = LineCase(name, pool, W, U, mode, starts, disp)
    _, track, _ = trial.twin_solution()
    K, ok = verdict(track), sure(track)
    good = {True: list(np.nonzero(ok & (K == W))[0]), False: list(np.nonzero(ok & (K < W))[0])}
    rows = []
    for n in range(N):
        want = n % 2 == 0
        if not good[want]:
            want = not want
        assert good[want], f"{name} N={N} W={W} U={U} mode={mode}: the pool has no query left"
        rows.append(good[want].pop(0))
    return trial.sub(np.array(rows))


# ---- the checks of a tracker's answer, the restatement's or the kernel's -----------------------------------------------------------
def left_out(case, q):
    """[...] bool: the poses the teacher-forced comparison leaves out (chain_ik_pose_common.left_out's rule, for the held goal)"""
    if case.mode == HOLD_POSITION:
        return np.zeros(q.shape[:-1], bool)
    p0, goal = case.held()
    R_ee, _ = case.twin.end_effector_frame(q)
    if case.mode == HOLD_AXIS:
        t = R_ee @ TOOL_AXIS
        return (np.linalg.norm(np.cross(t, goal), axis=-1) < 1e-2) & (np.sum(t * goal, axis=-1) < 0.0)
    _, angle = case.twin.pose_errors(q, p0, case.mode, goal, TOOL_AXIS, TOOL_NORMAL)
    return angle > np.pi - P.PI_BAND


def check_iterations(case, iters, nodes):
    """Teacher-forced: every recorded update against the twin's step applied to the recorded pose before it, towards the line point
    of its waypoint; the limits hold exactly; iters[0] is q_start and iters[i U] is node i, bit for bit; at most CAP of the updates
    are left out. Returns the largest deviation, max-norm over the joints, and the share left out."""
    model, twin, W, U, N = case.model, case.twin, case.W, case.U, case.N
    c = constants(model)
    assert iters.dtype == np.float32 and iters.shape == (W * U + 1, N, model.A)
    assert nodes.dtype == np.float32 and nodes.shape == (N, W + 1, model.A)
    assert np.array_equal(iters[0], case.q_start.astype(np.float32))
    assert np.array_equal(iters[::U].view(np.uint32), np.ascontiguousarray(nodes.transpose(1, 0, 2)).view(np.uint32))
    lo = np.array([j.lower if j.limited else -np.inf for j in model.joints]).astype(np.float32)
    hi = np.array([j.upper if j.limited else np.inf for j in model.joints]).astype(np.float32)
    assert np.all(iters[1:] >= lo) and np.all(iters[1:] <= hi)
    p0, goal = case.held()
    before = iters[:-1].astype(np.float64)
    i = np.arange(W * U) // U + 1
    g = p0[None] + (i / W)[:, None, None] * case.disp[None]
    if case.mode == HOLD_POSITION:
        want = twin.ik_step(before, g, c["lam"], c["e_max"], c["dq_max"])
    else:
        want = twin.ik_pose_step(before, g, case.mode, goal[None], c["lam"], c["e_max"], c["dq_max"], c["weight"], c["w_max"], TOOL_AXIS,
                                 TOOL_NORMAL)
    out = left_out(case, before)
    assert out.mean() <= CAP, (float(out.mean()), CAP)
    dev = np.abs(iters[1:].astype(np.float64) - want).max(axis=-1)
    return float(np.where(out, 0.0, dev).max()), float(out.mean())


def check_records(case, nodes, track):
    """Soundness, independent of the twin's tracker: the four floats against line_record in float64 at the returned nodes; [2]
    bit for bit against the float32 differences of the nodes; every waypoint of a tracked prefix within tolerance + 2 tol_of(model)
    of its line point and within orientation_tolerance + ANGLE_BOUND of the held orientation, by the twin. Returns the largest
    deviation of [0], [1], [3]."""
    model, twin, W = case.model, case.twin, case.W
    assert track.dtype == np.float32 and track.shape == (case.N, W, LM.TRACK_FLOATS)
    p0, goal = case.held()
    q = nodes.astype(np.float64)
    true = np.stack([LM.line_record(twin, q[:, i - 1], q[:, i], p0, case.disp, i, W, case.mode, goal, TOOL_AXIS, TOOL_NORMAL)
                     for i in range(1, W + 1)], axis=1)
    step = np.max(np.abs(nodes[:, 1:] - nodes[:, :-1]), axis=-1)
    assert step.dtype == np.float32 and np.array_equal(track[:, :, 2].view(np.uint32), step.view(np.uint32))
    if case.mode == HOLD_POSITION:
        assert not track[:, :, 1].any()
    dev = np.abs(track.astype(np.float64) - true).max(axis=(0, 1))
    K = verdict(track)
    inside = np.arange(W)[None, :] < K[:, None]
    tol = C.tol_of(model)
    assert np.all(true[:, :, 0][inside] <= TOLERANCE + 2 * tol)
    assert np.all(true[:, :, 1][inside] <= ORIENTATION_TOLERANCE + ANGLE_BOUND)
    return float(dev[0]), float(dev[1]), float(dev[3])


def check_verdict(case, track):
    """Completeness: K per query equals the twin's for every query whose twin verdict has room to spare; no query of a case is
    without it, by construction. Returns the census {'tracked': .., 'lost': ..}."""
    _, twin_track, _ = case.twin_solution()
    ok = sure(twin_track)
    assert (~ok).sum() <= CAP * case.N and not (~ok).any(), np.nonzero(~ok)[0]
    K, want = verdict(track), verdict(twin_track)
    assert np.array_equal(K[ok], want[ok]), (K, want)
    census = {"tracked": int(np.sum(K == case.W)), "lost": int(np.sum(K < case.W))}
    if case.N >= 64 and not (case.name == "slider4" and case.mode != HOLD_POSITION):
        assert min(census.values()) >= 1, f"vacuous: {census}"
    return census
