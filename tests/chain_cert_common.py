"""Shared by tests/test_chain_cert_cpu.py and tests/test_chain_cert_gpu.py: the cases that hold naf_chain_path_certify
(csrc/chain_env.hip) against the float64 rule of environment/kinematic.py (reach_table, path_half_steps, certify_joint_path), built
with the twin alone from chain_path_common's arms and counts; a float32 restatement of the half-steps and the record that stands in
for the device in the CPU rehearsal; and the checks both suites apply to what a checker — that restatement, or the kernel — returned."""
import functools

import numpy as np

import chain_box_common as BX
import chain_path_common as P
import chain_rollout_common as C

from robotic_manipulator_rloa_amd.environment.kinematic import (KinematicEnvironment, certificate_guard, check_joint_path,
                                                                joint_distance32, path_half_steps, path_pose, path_slacks, path_vias,
                                                                reach_table)

ORAD, CAP = P.ORAD, P.CAP
COUNTS, ARMS, EXTRA = P.COUNTS, P.ARMS, P.EXTRA
CASES = [(name, N, Cn, S) for name in ARMS for N, Cn, S in COUNTS] + EXTRA
FLOOR = C.FLOOR                    # certified candidates a 256-candidate case must hold, and as many blocked
UNCERTIFIED = 3                    # ... and candidates free at their samples yet uncertified: what a kernel that forgets beta gets wrong
BANDS = np.array([2.0, 4.0, 2.0])  # x tol: the obstacle's slack | the pairs' | the workcell's (chain_path_common.band_of's)


def f32(x):
    return C.f32(x)


def betas_of(case):
    """(beta_1, beta_2, beta_via) [N, C, n_seg + P] float64 of the case's candidates"""
    return path_half_steps(case.model, case.q_start[:, None, :], case.vias, case.q_goal[:, None, :], case.S)


def bounds_of(case):
    """[N, C, 3]: how far a float32 slack may lie from the twin's at the same pose — the clearance's own 2 tol / 4 tol / 2 tol, and
    2^-20 of the candidate's largest half-step for the float32 rounding of beta (A + 2 roundings of 2^-24 relative, A <= 12)"""
    tol = C.tol_of(case.model)
    return BANDS * tol + 2.0 ** -20 * betas_of(case)[2].max(axis=-1)[..., None]


def slacks_at(case, poses):
    """[N, C, S, 3] float64: the twin's three slacks at poses[N, C, S, A]"""
    return path_slacks(case.twin, np.asarray(poses, np.float64), case.obstacles[:, None, :], betas_of(case),
                       certificate_guard(case.model))


def band_of(case, slacks):
    """[N, C, S] bool: a sample one of whose twin slacks lies within bounds_of of the margin, where the device's verdict is not
    compared"""
    with np.errstate(invalid="ignore"):
        return np.any(np.abs(slacks - case.margin) <= bounds_of(case)[:, :, None, :], axis=-1)


def census_of(case):
    """(certified, blocked, free yet uncertified, samples in a band) of the case, by the twin alone at the restatement's poses"""
    poses = P.pose32(case.q_start[:, None, :], case.vias, case.q_goal[:, None, :], case.S)
    m, s = P.margins_at(case, poses), slacks_at(case, poses)
    blocked = np.any(m < case.margin, axis=-1).any(axis=-1)
    low = np.any(s < case.margin, axis=-1).any(axis=-1)
    return int((~low).sum()), int(blocked.sum()), int((low & ~blocked).sum()), int((band_of(case, s) | P.band_of(case, m)).sum())


@functools.lru_cache(maxsize=None)
def build(name, N, Cn, S):
    """chain_path_common.build_case, reseeded until the twin alone also meets, on a case of 256 candidates: at most CAP of the
    samples inside a band of either kind, FLOOR candidates certified, FLOOR blocked, UNCERTIFIED free at the samples yet uncertified"""
    for seed in range(20):
        case = P.build_case(name, N, Cn, S, seed=seed)
        if N * Cn < 256:
            return case
        certified, blocked, between, in_band = census_of(case)
        if in_band <= CAP * N * Cn * S and certified >= FLOOR and blocked >= FLOOR and between >= UNCERTIFIED:
            return case
    raise AssertionError(f"{name} N={N} C={Cn} S={S}: no seed meets the cap and the floors")


@functools.lru_cache(maxsize=None)
def boxes_without_pairs(N=4, Cn=4, S=128):
    """iiwa_like7 WITHOUT self-collision among chain_box_common's boxes: one wave per workgroup with CELL + BOX, the instantiation
    none of chain_path_common's arms launches. Built as build_case builds its cases, at iiwa_like7's margin; reseeded until the twin
    alone finds chain_path_common.floor_of candidates free and as many blocked, and no sample inside a band."""
    model = BX.model_of("iiwa_like7", workcell_boxes=BX.boxes_of("iiwa_like7"))
    twin = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), ORAD)
    assert not model.self_pairs and model.cell_boxes
    for attempt in range(40):
        rng = np.random.default_rng(4400 + attempt)
        q = P.IK.free_poses(model, twin, rng, 2 * N)
        a, b = q[:N], q[N:]
        vias = path_vias(model, a, b, Cn, seed=int(rng.integers(1 << 30))).astype(np.float64)
        ob = np.tile(C.away(model)[1], (N, 1))
        ob[1::2] = twin.end_effector(0.5 * (a + b))[1::2]
        case = P.Case("iiwa_like7", N, Cn, S, a, b, vias, f32(ob), margin=P.MARGINS["iiwa_like7"])
        case.name, case.model, case.twin = "iiwa_like7_boxes_no_pairs", model, twin
        poses = P.pose32(a[:, None, :], vias, b[:, None, :], S)
        m, s = P.margins_at(case, poses), slacks_at(case, poses)
        blocked = np.any(m < case.margin, axis=-1).any(axis=-1)
        if min(int(blocked.sum()), int((~blocked).sum())) >= P.floor_of(N, Cn) and not (band_of(case, s) | P.band_of(case, m)).any():
            return case
    raise AssertionError("iiwa_like7 among boxes without pairs: no seed meets the floors")


def beta32(case):
    """[3, N, C, n_seg + P] float32: the three tables as the kernel forms them — |b - a| in float32, the joint sum from 0 in joint
    order by fused multiply-add (the product of two float32 is exact in float64), one division by 2 n"""
    f = np.float32
    model, R = case.model, reach_table(case.model)
    n_seg = len(model.segments)
    a, v, b = f(case.q_start)[:, None, :], f(case.vias), f(case.q_goal)[:, None, :]
    h = case.S // 2
    out = np.zeros((3,) + v.shape[:-1] + (n_seg + len(model.self_pairs),), f)
    spans = [(s, 0, model.segments[s].frame) for s in range(n_seg)]
    spans += [(t, model.segments[s].frame, model.segments[t].frame) for s, t in model.self_pairs]
    for leg, (d, n) in enumerate(((np.abs(v - a), 2 * h), (np.abs(b - v), 2 * (h - 1)))):
        assert d.dtype == f
        for e, (s, m0, m1) in enumerate(spans):
            acc = np.zeros(v.shape[:-1], f)
            for m in range(m0, m1):
                acc = (d[..., m].astype(np.float64) * np.float64(R[m, s]) + acc.astype(np.float64)).astype(f)
            out[leg][..., e] = acc / f(n)
    out[2] = np.maximum(out[0], out[1])
    return out


def record32(case):
    """What naf_chain_path_certify returns, by the restatement: (out[N C, 12] float32, poses[N C, S, A] float32) — chain_path_common's
    record32, then the twin's per-test clearances at pose32's poses with beta32's entries and the guard subtracted, rounded to float32"""
    N, Cn, S = case.N, case.C, case.S
    out8, poses = P.record32(case)
    b = beta32(case).astype(np.float64)
    slack = path_slacks(case.twin, poses.reshape(N, Cn, S, -1).astype(np.float64), case.obstacles[:, None, :], (b[0], b[1], b[2]),
                        certificate_guard(case.model)).astype(np.float32)
    low = np.any(slack < np.float32(case.margin), axis=-1)
    out = np.empty((N * Cn, 12), np.float32)
    out[:, :8] = out8
    out[:, 8:11] = slack.min(axis=2).reshape(N * Cn, 3)
    out[:, 11] = np.where(low.any(axis=-1), np.argmax(low, axis=-1), -1).reshape(N * Cn)
    return out, poses


def check_records(case, out, poses):
    """The teacher-forced test of one case's twelve floats. [0 .. 7] go through chain_path_common.check_records unchanged. With the
    twin's slacks AT THE RECORDED POSES: [8] [9] [10] within bounds_of; [11] the twin's for every candidate none of whose samples
    lies inside a band, and between the first sample that may be low and the first that surely is where some do (at most CAP of
    the case's samples). A certified candidate has [4] == 0. Returns the census."""
    model, N, Cn, S = case.model, case.N, case.C, case.S
    assert out.dtype == np.float32 and out.shape == (N * Cn, 12)
    P.check_records(case, np.ascontiguousarray(out[:, :8]), poses)
    s = slacks_at(case, poses.reshape(N, Cn, S, -1))
    rec, bound = out.reshape(N, Cn, 12), bounds_of(case)
    for k in range(3):
        got, want = rec[..., 8 + k].astype(np.float64), s[..., k].min(axis=2)
        both_inf = np.isposinf(got) & np.isposinf(want)
        err = np.abs(np.where(both_inf, 0.0, got) - np.where(both_inf, 0.0, want))
        print(f"{case.name} N={N} C={Cn} S={S}: slack {k} off by {float(err.max()):.2e} at most (bound {float(bound[..., k].min()):.2e})")
        assert np.all(err <= bound[..., k]), (k, float(err.max()), float(bound[..., k].min()))
    if not model.self_pairs:
        assert np.all(np.isposinf(rec[..., 9]))
    if not model.cell_pairs:
        assert np.all(np.isposinf(rec[..., 10]))
    band = band_of(case, s)
    low = np.any(s < case.margin, axis=-1)
    sure, maybe = low & ~band, low | band
    assert band.sum() <= CAP * N * Cn * S, (int(band.sum()), N * Cn * S)
    first_of = lambda b: np.where(b.any(axis=-1), np.argmax(b, axis=-1), S)      # noqa: E731
    got_first = np.where(rec[..., 11] < 0, S, rec[..., 11]).astype(np.int64)
    assert np.all((first_of(maybe) <= got_first) & (got_first <= first_of(sure)))
    clean = ~band.any(axis=-1)
    assert np.array_equal(rec[..., 11][clean], np.where(low.any(axis=-1), np.argmax(low, axis=-1), -1)[clean])
    certified = rec[..., 11] == -1
    assert np.all(rec[..., 4][certified] == 0)
    census = dict(certified=int(certified.sum()), blocked=int(np.sum(rec[..., 4] > 0)),
                  between=int(np.sum(~certified & (rec[..., 4] == 0))), in_band=int(band.sum()))
    print(f"{case.name} N={N} C={Cn} S={S}: {census}")
    if N * Cn >= 256:
        assert census["certified"] >= FLOOR and census["blocked"] >= FLOOR and census["between"] >= UNCERTIFIED, f"vacuous: {census}"
    return census


def dense_margins(twin, a, via, b, obstacle, K):
    """[n, K, 3]: the twin's three clearances (the obstacle's minus its radius) at K uniformly spaced poses of each polyline
    a[n] -> via[n] -> b[n], the end poses included"""
    t = np.linspace(0.0, 2.0, K)[None, :, None]
    q = np.where(t <= 1.0, a[:, None, :] + t * (via - a)[:, None, :], via[:, None, :] + (t - 1.0) * (b - via)[:, None, :])
    clear = twin.clearance(q, obstacle[:, None, :]) - twin.obstacle_radius
    zero = np.zeros(clear.shape)
    return np.stack([clear, twin.self_clearance(q) + zero, twin.cell_clearance(q) + zero], axis=-1)


def missed_contact():
    """The contact the samples miss: planar3, S = 64, ONE straight candidate whose sample step is at least 0.05 rad; the obstacle's
    centre sits on the end effector's position midway between samples 10 and 11. The end effector travels some 15 mm over that half
    interval, less than the 30 mm radius of its capsule, so with margin 0 no obstacle there leaves the two samples free: the margin is
    minus that radius — the obstacle against the capsules' AXES — and the obstacle's radius, found with the twin, is half of what the
    nearer of the two samples' axes keeps from the centre. Both samples, and every other, are then free, and the midpoint, whose axis
    passes through the centre, is not. Returns (case, obstacle radius): the case's twin has that radius."""
    model, twin = P.arm("planar3")
    rng = np.random.default_rng(5)
    S, margin = 64, -float(np.float32(model.segments[-1].radius))
    for _ in range(400):
        a, b = (f32(P.IK.free_poses(model, twin, rng, 1)[0]) for _ in range(2))
        via = path_vias(model, a[None], b[None], 1, 0)[0, 0].astype(np.float64)
        if joint_distance32(b, a) / np.float32(31) < 0.05:
            continue
        q = path_pose(a, via, b, np.array([10, 11]), S)
        centre = f32(twin.end_effector(0.5 * (q[0] + q[1])))
        near = min(float(twin.clearance(q[0], centre)), float(twin.clearance(q[1], centre))) - margin      # (the axis to the centre)
        orad = float(np.float32(0.5 * near))
        if orad < 2e-3:
            continue
        case = P.Case("planar3", 1, 1, S, a[None], b[None], via[None, None], centre[None], margin=margin)
        case.twin = KinematicEnvironment(model, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), orad)
        rec = check_joint_path(case.twin, a, via, b, centre, S, margin)
        if rec[4] == 0 and min(rec[0], rec[2]) - margin > 8 * C.tol_of(model):
            return case, orad
    raise AssertionError("no straight path whose samples all stay clear of the end effector's position between samples 10 and 11")
