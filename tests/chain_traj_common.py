"""Shared by tests/test_chain_traj_cpu.py and tests/test_chain_traj_gpu.py: the cases that hold naf_chain_traj_check and
naf_chain_traj_certify (csrc/chain_env.hip) against the float64 rule of environment/trajectory.py (trajectory_law, check_trajectory,
trajectory_half_steps), built with the twin alone; a float32 restatement of the device's evaluation that stands in for it in the CPU
rehearsal; the checks both suites apply to what a checker — that restatement, or the kernel — returned; and the scene in which a
blended corner is blocked where its polyline is certified."""
import functools

import numpy as np

import chain_cert_common as K
import chain_ik_common as IK
import chain_roadmap_common as R
import chain_rollout_common as C

from robotic_manipulator_rloa_amd.environment import trajectory as T
from robotic_manipulator_rloa_amd.environment.kinematic import KinematicEnvironment, certificate_guard, path_slacks, reach_table

ORAD, CAP = R.ORAD, R.CAP
FLOOR, UNCERTIFIED, BANDS = K.FLOOR, K.UNCERTIFIED, K.BANDS
DT = 1.0 / 240.0
# (arm, N, legs, S). Every arm: three trajectories of one leg in one pass; five of two legs in two passes; 64 of five legs, where
# the floors hold. iiwa_like7 also at 63 legs and S = 2112 > 2048; the last two arms complete the six instantiations of the pack.
# Trajectory 0 of every case has S_n = S exactly, trajectory 1 S_n = S - 63, trajectory 2 is ONE node: a single sample.
COUNTS = [(3, 1, 64), (5, 2, 128), (64, 5, 128)]
CASES = [(name, N, L, S) for name in R.ARMS for N, L, S in COUNTS] + [("iiwa_like7", 4, 63, 2112), ("iiwa_like7_bare", 4, 2, 128),
                                                                     ("planar3_boxes", 4, 5, 128)]
# how far a case's nodes lie from their query's seeded free pose, per joint at most (rad or m): long12 and iiwa_like7 live
# millimetres from themselves and their boxes, and a certified trajectory has to keep beta on top of the margin
SPREAD = {"planar3": 0.5, "slider4": 0.3, "iiwa_like7": 0.12, "long12": 0.07, "iiwa_like7_bare": 0.3, "planar3_boxes": 0.3}
MARGINS = dict(R.MARGINS, long12=-0.006)

# The pose bound. test_chain_traj_cpu.test_rehearsal measures, over every live sample of every case, the largest deviation of the
# float32 restatement's pose (law32) from trajectory_law in float64 on the same float32 schedule:
#     planar3 2.32e-7, iiwa_like7 2.36e-7 (2.36e-7 at 63 legs and 2112 ticks), long12 1.21e-7, slider4 2.28e-7,
#     iiwa_like7_bare 1.11e-7, planar3_boxes 2.43e-7   ->   POSE_DEVIATION = 2.5e-7, rounded up
# — the rounding of t = (float)i dt and of s (2^-24 of up to 9 s, times a joint speed of up to a few rad/s), of the three velocities
# and of the blend coefficients: about one ulp of a joint value of 3 rad. The bound is 4 x the measured value: the restatement rounds every product and sum once where the
# compiler may contract a product into the sum that follows it. It is taken from the restatement, never from the kernel.
POSE_DEVIATION = 2.5e-7
POSE_BOUND = 4 * POSE_DEVIATION


def f32(x):
    return C.f32(x)


class Case:
    """N trajectories of one arm at S ticks of dt: the float32 schedule `ds` (trajectory.DeviceSchedule), obstacles[N, 3] (float32
    values held as float64), margin. E = 1 and V let chain_roadmap_common's margins_at / band_of read it."""
    E = 1

    def __init__(self, name, S, ds, obstacles, margin):
        self.name, self.S, self.ds, self.obstacles, self.margin = name, S, ds, obstacles, margin
        self.model, self.twin = R.arm(name)
        self.N, self.V, self.dt = len(ds.n_nodes), ds.nodes.shape[1], ds.dt
        self.live = np.arange(S)[None, :] < ds.n_samples[:, None]


def law64(ds, S):
    return T.trajectory_poses(ds, S)


def _fma(a, b, c):
    """float32 fmaf of float32 arrays: the product is exact in float64, the sum is rounded there and once more to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def law32(ds, S):
    """[N, S, A] float32: every tick's pose as the device forms it (TrajLine::sample and ::pose), operation by operation in float32"""
    f = np.float32
    N, V, A = ds.nodes.shape
    tk, tau, iT = (ds.times[..., k][:, None, :] for k in range(3))                       # [N, 1, V]
    n = ds.n_nodes.astype(np.int64)[:, None]
    Kl = n - 1
    t = np.broadcast_to((np.arange(S).astype(f) * f(ds.dt)).astype(f), (N, S))
    j = np.sum((np.arange(V)[None, None, :] < n[..., None]) & (tk <= t[..., None]), axis=-1)
    at = lambda x, k: np.take_along_axis(np.broadcast_to(x, (N, S, V)), k[..., None], axis=-1)[..., 0]      # noqa: E731
    jp, jn, jq = np.maximum(j - 1, 0), np.minimum(j, Kl), np.minimum(j + 1, Kl)
    zero = np.zeros((N, S), f)
    s = t - np.where(j >= 1, at(tk, jp), zero)
    tau_p, tau_n = np.where(j >= 1, at(tau, jp), zero), np.where(j <= Kl, at(tau, jn), zero)
    h0 = np.maximum(zero, f(0.5) * tau_p - s)
    h1 = np.where(j <= Kl, np.maximum(zero, (t - at(tk, jn)) + f(0.5) * tau_n), zero)
    with np.errstate(divide="ignore", invalid="ignore"):
        c0 = np.where(tau_p > 0, f(0.5) * h0 * h0 * (f(1.0) / tau_p), zero)
        c1 = np.where(tau_n > 0, f(0.5) * h1 * h1 * (f(1.0) / tau_n), zero)
    wm = np.where(j >= 2, at(iT, jp), zero)
    w = np.where((j >= 1) & (j <= Kl), at(iT, jn), zero)
    wp = np.where(j + 1 <= Kl, at(iT, jq), zero)
    assert all(x.dtype == f for x in (t, s, h0, h1, c0, c1, wm, w, wp))
    node = lambda k: np.take_along_axis(ds.nodes[:, None], np.broadcast_to(k[..., None, None], (N, S, 1, A)), axis=2)[:, :, 0]  # noqa: E731
    pm2, pm1, p0, p1 = node(np.maximum(j - 2, 0)), node(np.maximum(j - 1, 0)), node(jn), node(jq)
    v_prev, v, v_next = (pm1 - pm2) * wm[..., None], (p0 - pm1) * w[..., None], (p1 - p0) * wp[..., None]
    q = _fma(v, np.broadcast_to(s[..., None], v.shape), pm1)
    q = _fma(np.broadcast_to(c0[..., None], v.shape), v - v_prev, q)
    return _fma(np.broadcast_to(c1[..., None], v.shape), v_next - v, q)


# ---- building cases ----------------------------------------------------------------------------------------------------------------
def schedules_for(polys, durations, dt, vmax=1.0, amax=4.0):
    """blend_schedule of every polyline, its limits scaled so that it lasts durations[n] (None: as scheduled): a time scaling by c is
    the schedule under vmax / c and amax / c^2"""
    out = []
    for poly, D in zip(polys, durations):
        A = poly.shape[1]
        s = T.blend_schedule(poly, np.full(A, vmax), np.full(A, amax))
        if D is not None and s["duration"] > 0.0:
            c = D / s["duration"]
            s = T.blend_schedule(poly, np.full(A, vmax / c), np.full(A, amax / (c * c)))
        out.append(s)
    return out


def local_case(name, N, L, S, seed):
    """The nodes of query n lie within SPREAD of ONE seeded free pose (clipped into the limits, float32 values). Every second query's
    obstacle, from query 1 on, sits on the end effector of its first leg's middle pose; the others' is out of the way (for an arm
    without a workcell, every fourth's on the end effector of a pose beside the polyline). Durations: query 0 fills the launch
    (S_n = S), query 1 has S_n = S - 63, query 2 is one node; the others last a random share of the launch, short ones driven fast
    (a large beta: free yet uncertified) and long ones slowly."""
    model, twin = R.arm(name)
    rng = np.random.default_rng(8800 + 131 * N + 17 * L + S + 10007 * seed)
    centre = IK.free_poses(model, twin, rng, N)
    lo, hi = C.limits_of(model)
    spread = SPREAD[name] / (1.0 if L < 63 else 4.0)
    nodes = f32(np.clip(centre[:, None, :] + rng.uniform(-spread, spread, (N, L + 1, model.A)), lo, hi))
    if N > 2:
        nodes[2] = nodes[2, :1]                                               # a single node, L + 1 times: one sample
    ob = np.tile(C.away(model)[1], (N, 1))
    ob[1::2] = twin.end_effector(0.5 * (nodes[:, 0] + nodes[:, 1]))[1::2]
    if not model.cell_pairs:
        ob[0::4] = (twin.end_effector(nodes[:, 0]) + [0.0, 0.0, ORAD + 0.08])[0::4]
    share = np.exp(rng.uniform(np.log(0.04), 0.0, N))
    durations = [(S - 2.5) * DT * u for u in share]
    durations[0] = (S - 1.5) * DT
    if N > 1:
        durations[1] = (S - 64.5) * DT if S > 64 else 0.5 * DT      # (S_n = S - 63; at S = 64 that is the one sample query 2 has: 2 here)
    ds = T.device_schedule(schedules_for(list(nodes), durations, DT), DT, L + 1 if L >= 1 else 2)
    return Case(name, S, ds, f32(ob), MARGINS.get(name, 0.0))


def betas_of(case):
    return T.trajectory_half_steps(case.model, case.ds.vpeak, case.dt)


def bounds_of(case):
    """[N, 1, 3]: how far a float32 slack may lie from the twin's at the same pose (chain_edgecert_common.bounds_of's rule)"""
    return (BANDS * C.tol_of(case.model) + 2.0 ** -20 * betas_of(case).max(axis=-1)[..., None])[:, None, :]


def slacks_at(case, poses, beta=None):
    """[N, 1, S, 3] float64: the twin's three slacks at poses[N, S, A]"""
    b = betas_of(case) if beta is None else beta
    return path_slacks(case.twin, np.asarray(poses, np.float64), case.obstacles, (b, b, b), certificate_guard(case.model))[:, None]


def margins_at(case, poses):
    return R.margins_at(case, np.asarray(poses)[:, None])                     # [N, 1, S, 3]


def slack_band_of(case, slacks):
    with np.errstate(invalid="ignore"):
        return np.any(np.abs(slacks - case.margin) <= bounds_of(case)[:, :, None, :], axis=-1)


def census_of(case, poses):
    """(certified, blocked, free yet uncertified, live samples in a band) by the twin alone at the given poses"""
    m, s = margins_at(case, poses)[:, 0], slacks_at(case, poses)[:, 0]
    live = case.live
    blocked = (np.any(m < case.margin, axis=-1) & live).any(axis=-1)
    low = (np.any(s < case.margin, axis=-1) & live).any(axis=-1)
    band = (slack_band_of(case, s[:, None])[:, 0] | R.band_of(case, m[:, None])[:, 0]) & live
    return int((~low).sum()), int(blocked.sum()), int((low & ~blocked).sum()), int(band.sum())


# Which seed build() accepted for each case of 64 trajectories: test_chain_traj_cpu.test_rehearsal finds it with the twin
# (verify=True) and holds this table to it; the GPU suite builds the same case without asking the twin a second time — check_records
# asserts the cap and the floors again, at the recorded poses.
SEED = {("planar3", 64, 5, 128): 0, ("iiwa_like7", 64, 5, 128): 0, ("long12", 64, 5, 128): 0, ("slider4", 64, 5, 128): 0}


@functools.lru_cache(maxsize=None)
def build(name, N, L, S, verify=True):
    """local_case, for a case of 64 trajectories reseeded until the twin alone meets, at the restatement's poses: at most CAP of the
    live samples inside a band of either kind, FLOOR trajectories certified, FLOOR blocked, UNCERTIFIED free at the ticks yet
    uncertified. verify=False builds SEED's without asking the twin."""
    if N < 64:
        return local_case(name, N, L, S, 0)
    for seed in range(20) if verify else [SEED[(name, N, L, S)]]:
        case = local_case(name, N, L, S, seed)
        case.seed = seed
        if not verify:
            return case
        certified, blocked, between, in_band = census_of(case, law32(case.ds, S))
        if in_band <= CAP * case.live.sum() and certified >= FLOOR and blocked >= FLOOR and between >= UNCERTIFIED:
            return case
    raise AssertionError(f"{name} N={N} L={L} S={S}: no seed meets the cap and the floors")


# ---- the restatement's record ------------------------------------------------------------------------------------------------------
def spans_of(model):
    n_seg = len(model.segments)
    return ([(s, 0, model.segments[s].frame) for s in range(n_seg)] +
            [(t, model.segments[s].frame, model.segments[t].frame) for s, t in model.self_pairs])


def beta32(case):
    """[N, n_seg + P] float32: the table as the kernel forms it — the joint sum from 0 in joint order by fmaf, then times (0.5f dt)"""
    f = np.float32
    Rt, vp = reach_table(case.model), case.ds.vpeak
    out = np.zeros((case.N, len(spans_of(case.model))), f)
    for e, (s, m0, m1) in enumerate(spans_of(case.model)):
        acc = np.zeros(case.N, f)
        for m in range(m0, m1):
            acc = _fma(vp[:, m], np.full(case.N, Rt[m, s], f), acc)
        out[:, e] = (f(0.5) * f(case.dt)) * acc
    return out


def record32(case, certify=True):
    """What the launch returns, by the restatement: (out[N, 12 | 8] float32, poses[N, S, A] float32)"""
    N, S, ds, live = case.N, case.S, case.ds, case.live
    poses = law32(ds, S)
    m = margins_at(case, poses)[:, 0].astype(np.float32)
    blocked = np.any(m < np.float32(case.margin), axis=-1) & live
    out = np.empty((N, 12 if certify else 8), np.float32)
    out[:, :3] = np.where(live[..., None], m, np.inf).min(axis=1)
    out[:, 3] = np.where(blocked.any(axis=1), np.argmax(blocked, axis=1), -1)
    out[:, 4] = blocked.sum(axis=1)
    last = ds.times[np.arange(N), ds.n_nodes - 1]
    out[:, 5] = last[:, 0] + np.float32(0.5) * last[:, 1]
    out[:, 6] = (ds.vpeak * np.float32(ds.dt)).max(axis=1)
    out[:, 7] = blocked[np.arange(N), ds.n_samples - 1]
    if certify:
        slack = slacks_at(case, poses, beta32(case).astype(np.float64))[:, 0].astype(np.float32)
        low = np.any(slack < np.float32(case.margin), axis=-1) & live
        out[:, 8:11] = np.where(live[..., None], slack, np.inf).min(axis=1)
        out[:, 11] = np.where(low.any(axis=1), np.argmax(low, axis=1), -1)
    return out, poses


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def check_poses(case, poses):
    """poses[N, S, A] float32 within POSE_BOUND of the float64 law at every live sample; the rows i >= S_n ARE the last node, bit for
    bit, and so is sample 0 the first. Returns the largest deviation."""
    ds, S = case.ds, case.S
    assert poses.dtype == np.float32 and poses.shape == (case.N, S, case.model.A)
    want = law64(ds, S)
    dev = float(np.abs(np.where(case.live[..., None], poses.astype(np.float64) - want, 0.0)).max())
    print(f"{case.name} N={case.N} V={case.V} S={S}: largest pose deviation {dev:.2e} (bound {POSE_BOUND:.2e})")
    assert dev <= POSE_BOUND, (dev, POSE_BOUND)
    last = ds.nodes[np.arange(case.N), ds.n_nodes - 1]
    dead = ~case.live
    assert np.array_equal(poses[dead].view(np.uint32), np.broadcast_to(last[:, None, :], poses.shape)[dead].view(np.uint32))
    assert np.array_equal(poses[:, 0].view(np.uint32), ds.nodes[:, 0].view(np.uint32))
    return dev


def _bracket(rec_first, rec_count, flag, band, live, S):
    """chain_roadmap_common.check_records' rule for a first index and a count, over the live samples only"""
    flag, band = flag & live, band & live
    sure, maybe = flag & ~band, flag | band
    first_of = lambda x: np.where(x.any(axis=-1), np.argmax(x, axis=-1), S)      # noqa: E731
    got_first = np.where(rec_first < 0, S, rec_first).astype(np.int64)
    assert np.all((first_of(maybe) <= got_first) & (got_first <= first_of(sure)))
    if rec_count is not None:
        assert np.all((sure.sum(axis=-1) <= rec_count) & (rec_count <= maybe.sum(axis=-1)))
    clean = ~band.any(axis=-1)
    assert np.array_equal(rec_first[clean], np.where(flag.any(axis=-1), np.argmax(flag, axis=-1), -1)[clean])
    if rec_count is not None:
        assert np.array_equal(rec_count[clean], flag.sum(axis=-1)[clean])
    return clean


def check_records(case, out, poses, certify=True):
    """The teacher-forced test of one case's records, with the twin evaluated AT THE RECORDED POSES over the LIVE samples only:
    [0] [1] [2] within 2 tol / 4 tol / 2 tol (+inf without pairs / a workcell); [3] [4] the twin's for every trajectory none of
    whose live samples lies inside a band, bracketed by its sure and possible samples otherwise; [5] [6] bit-equal to the float32
    formulas; [7] the twin's verdict on sample S_n - 1 unless that sample is in a band; certify: [8] [9] [10] within
    chain_edgecert_common's bounds, [11] by the same bracket; a certified trajectory has [4] == 0. At most CAP of the live samples
    lie inside a band; a case of 64 holds the three kinds. Returns the census."""
    model, N, S, ds, live = case.model, case.N, case.S, case.ds, case.live
    tol = C.tol_of(model)
    assert out.dtype == np.float32 and out.shape == (N, 12 if certify else 8)
    m = margins_at(case, poses)[:, 0]
    for k, bound in ((0, 2 * tol), (1, 4 * tol), (2, 2 * tol)):
        got, want = out[:, k].astype(np.float64), np.where(live, m[..., k], np.inf).min(axis=1)
        both_inf = np.isposinf(got) & np.isposinf(want)
        err = np.abs(np.where(both_inf, 0.0, got) - np.where(both_inf, 0.0, want))
        assert np.all(err <= bound), (k, float(err.max()), bound)
    if not model.self_pairs:
        assert np.all(np.isposinf(out[:, 1]))
    if not model.cell_pairs:
        assert np.all(np.isposinf(out[:, 2]))
    last = ds.times[np.arange(N), ds.n_nodes - 1]
    assert np.array_equal(out[:, 5].view(np.uint32), (last[:, 0] + np.float32(0.5) * last[:, 1]).view(np.uint32))
    assert np.array_equal(out[:, 6].view(np.uint32), (ds.vpeak * np.float32(ds.dt)).max(axis=1).view(np.uint32))
    band = R.band_of(case, m[:, None])[:, 0]
    blocked = np.any(m < case.margin, axis=-1)
    assert (band & live).sum() <= CAP * live.sum(), (int((band & live).sum()), int(live.sum()))
    _bracket(out[:, 3], out[:, 4], blocked, band, live, S)
    at_last = (np.arange(N), ds.n_samples - 1)
    sure_last = ~band[at_last]
    assert np.array_equal(out[:, 7][sure_last], blocked[at_last][sure_last].astype(np.float32))
    census = dict(free=int(np.sum(out[:, 4] == 0)), blocked=int(np.sum(out[:, 4] > 0)), in_band=int((band & live).sum()))
    if certify:
        s = slacks_at(case, poses)[:, 0]
        bound = bounds_of(case)[:, 0]
        for k in range(3):
            got, want = out[:, 8 + k].astype(np.float64), np.where(live, s[..., k], np.inf).min(axis=1)
            both_inf = np.isposinf(got) & np.isposinf(want)
            err = np.abs(np.where(both_inf, 0.0, got) - np.where(both_inf, 0.0, want))
            assert np.all(err <= bound[:, k]), (k, float(err.max()), float(bound[:, k].min()))
        sband = slack_band_of(case, s[:, None])[:, 0]
        assert (sband & live).sum() <= CAP * live.sum(), (int((sband & live).sum()), int(live.sum()))
        _bracket(out[:, 11], None, np.any(s < case.margin, axis=-1), sband, live, S)
        certified = out[:, 11] == -1
        assert np.all(out[:, 4][certified] == 0)
        census.update(certified=int(certified.sum()), between=int(np.sum(~certified & (out[:, 4] == 0))), in_slack_band=int((sband & live).sum()))
    print(f"{case.name} N={N} V={case.V} S={S}: {census}")
    if N >= 64:
        assert census["blocked"] >= FLOOR, f"vacuous: {census}"
        if certify:
            assert census["certified"] >= FLOOR and census["between"] >= UNCERTIFIED, f"vacuous: {census}"
    return census


# ---- dead samples do not count -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dead_end_case(S=128):
    """planar3, two trajectories of one leg that last a quarter of the launch. The obstacle of trajectory 0 sits ON the end effector
    of its last node, and the margin (negative: an allowed overlap, found with the twin) lies midway between the clearance of the
    last live sample and that of the one before it — every live sample before the last is free, the last is blocked, and the 3/4
    of the launch behind it evaluates to that blocked pose. Trajectory 1 is the same with the obstacle away: free."""
    model, twin = R.arm("planar3")
    rng = np.random.default_rng(11)
    tol = C.tol_of(model)
    for _ in range(200):
        a, b = (f32(IK.free_poses(model, twin, rng, 1)[0]) for _ in range(2))
        ds = T.device_schedule(schedules_for([np.stack([a, b])] * 2, [(S // 4 - 1.5) * DT] * 2, DT), DT, 2)
        q = law64(ds, S)[0, :ds.n_samples[0]]
        centre = f32(twin.end_effector(q[-1]))
        clear = twin.clearance(q, centre) - ORAD
        margin = float(np.float32(0.5 * (clear[-1] + clear[-2])))
        if clear[:-1].min() - margin < 16 * tol or margin - clear[-1] < 16 * tol or np.min(twin.cell_clearance(q)) < 1e-3:
            continue
        return Case("planar3", S, ds, np.stack([centre, f32(C.away(model)[1])]), margin)
    raise AssertionError("no leg whose last pose alone is below a margin")


# ---- the corner: certified as a polyline, blocked when blended -----------------------------------------------------------------------
CORNER = dict(margin=0.01, amax=1.0, fast=1.0, slow=0.2, orad=0.01)


class PolylinePaths:
    """what edge_certificate.polyline_nodes reads of a JointPaths, for one-via polylines start -> via -> goal given by hand"""

    def __init__(self, nodes):
        nodes = np.asarray(nodes, np.float64)
        self.start, self.via, self.goal = nodes[:, 0], nodes[:, 1], nodes[:, 2]
        self.candidate, self.n_nodes, self.nodes = np.ones(len(nodes), np.int64), np.zeros(len(nodes), np.int64), None


@functools.lru_cache(maxsize=None)
def corner_scene():
    """planar3 without a workcell on a two-leg polyline P_0 -> P_1 -> P_2: the base joint sweeps through at a constant speed while
    the elbow folds and unfolds, so P_1 is the most folded pose. Blended at CORNER's fast speed the arm is at the base angle of P_1
    with its elbow |v_2 - v_1| tau_1 / 8 = v^2 / (2 amax) = 0.5 rad LESS folded — its end effector reaches where no pose of the
    polyline does. A small sphere (radius CORNER['orad']) is put on the end effector of THAT pose, q(t_1): the polyline keeps 3 cm
    from it, the blended trajectory runs through it, and at the slow speed the deviation is 25 x smaller and the trajectory is back
    beside its polyline. Returns (model, twin with that radius, paths, obstacle[1, 3])."""
    model, _ = C.arm("planar3", False)
    twin = KinematicEnvironment(model, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), CORNER["orad"])
    P = f32(np.array([[-1.6, 0.6, 0.0], [0.0, 2.2, 0.0], [1.6, 0.6, 0.0]]))
    s = T.blend_schedule(P, np.full(3, CORNER["fast"]), np.full(3, CORNER["amax"]))
    apex = T.law_of(s, [s["node_times"][1]])[0]
    return model, twin, PolylinePaths(P[None]), f32(twin.end_effector(apex))[None]
