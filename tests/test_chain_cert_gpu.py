"""GPU (`-m gpu`): naf_chain_path_certify (csrc/chain_env.hip) against the float64 rule of environment/kinematic.py (reach_table,
path_half_steps, certify_joint_path) and against naf_chain_path_check on the same inputs, through the C ABI; chain_tools.JointPathChecker
(certify=True) and ManipulatorFramework.plan_joint_paths(certify=True) against joint_paths_host(certify=True).
tests/test_chain_cert_cpu.py rehearses every case with a float32 restatement."""
import ctypes

import numpy as np
import pytest
import torch

import chain_cert_common as K
import chain_path_common as P
import chain_rollout_common as C
from test_chain_path_gpu import PAD, PathRig, bits
from test_chain_rollout_gpu import IIWA_RANGED

from robotic_manipulator_rloa_amd.environment.kinematic import (JointPaths, certificate_guard, certify_joint_path, joint_paths_host,
                                                                reach_table)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class CertRig:
    """The certifying launch of one case through the C ABI; out and poses_out have PAD poisoned candidates behind the launch's."""

    def __init__(self, case, orad=P.ORAD):
        from robotic_manipulator_rloa_amd import _lib
        self.lib, self.case, self.orad = _lib.load(), case, float(np.float32(orad))
        model = case.model
        self.K, self.S, self.A = case.N * case.C, case.S, model.A
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)      # noqa: E731
        self.q_start, self.q_goal, self.obstacles = dev(case.q_start), dev(case.q_goal), dev(case.obstacles)
        self.vias = dev(case.vias.reshape(self.K, self.A))
        self.reach, self.guard = dev(reach_table(model)), certificate_guard(model)
        nan = dict(fill_value=float("nan"), device=DEV)
        self.out = torch.full((self.K + PAD, 12), **nan)
        self.poses = torch.full((self.K + PAD, self.S, self.A), **nan)

    def call(self, poses=True, **kw):
        """the entry point's return code, with arguments replaced by kw"""
        p = lambda t: t.data_ptr()      # noqa: E731
        case = self.case
        a = dict(h=self.h, a=p(self.q_start), b=p(self.q_goal), v=p(self.vias), o=p(self.obstacles), rad=self.orad, reach=p(self.reach),
                 guard=self.guard, N=case.N, Cn=case.C, S=case.S, margin=case.margin, out=p(self.out),
                 poses=p(self.poses) if poses else None)
        a.update(kw)
        return self.lib.naf_chain_path_certify(a["h"], a["a"], a["b"], a["v"], a["o"], a["rad"], a["reach"], a["guard"], a["N"], a["Cn"],
                                               a["S"], a["margin"], a["out"], a["poses"], torch.cuda.current_stream().cuda_stream)

    def run(self, poses=True):
        """returns (out[N C, 12], poses[N C, S, A]) as numpy copies"""
        self.out.fill_(float("nan"))
        assert self.call(poses) == 0
        torch.cuda.synchronize()
        assert torch.isnan(self.out[self.K:]).all() and torch.isnan(self.poses[self.K:]).all()
        return self.out[:self.K].cpu().numpy(), self.poses[:self.K].cpu().numpy()

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


@pytest.mark.parametrize("name,N,Cn,S", K.CASES)
def test_certify_against_the_rule_and_the_sampled_check(name, N, Cn, S):
    """One case through the C ABI, poses_out on. Teacher-forced (chain_cert_common.check_records): [0 .. 7] pass
    chain_path_common.check_records unchanged; the twin's slacks AT THE RECORDED POSES give [8] [9] [10] within 2 tol / 4 tol / 2 tol
    + 2^-20 beta and [11] wherever no sample lies inside a band; a 256-candidate case holds certified, blocked and
    free-yet-uncertified candidates. Parity with naf_chain_path_check on the same inputs: [5] bit-equal,
    [6] within an ulp, the three minima within 1 tol (what kernels of two shapes differ by, NOTEBOOK §22), [3] [4] [7] equal for
    every candidate none of whose samples lies inside a band. A run without poses_out gives the same bits; the PAD rows keep their
    poison."""
    case = K.build(name, N, Cn, S)
    rig = CertRig(case)
    out, poses = rig.run()
    plain, _ = rig.run(poses=False)
    rig.close()
    old = PathRig(case)
    out8, poses8 = old.run()
    old.close()
    assert np.array_equal(bits(out), bits(plain))
    K.check_records(case, out, poses)
    print(f"{name} N={N} C={Cn} S={S}: poses {'bit-equal' if np.array_equal(bits(poses), bits(poses8)) else 'differ'}")
    assert np.array_equal(bits(out[:, 5]), bits(out8[:, 5]))
    assert np.all(np.abs(out[:, 6] - out8[:, 6]) <= np.spacing(out8[:, 6]))
    tol = C.tol_of(case.model)
    for k in range(3):
        got, want = out[:, k].astype(np.float64), out8[:, k].astype(np.float64)
        both_inf = np.isposinf(got) & np.isposinf(want)
        err = float(np.abs(np.where(both_inf, 0.0, got) - np.where(both_inf, 0.0, want)).max())
        print(f"{name} N={N} C={Cn} S={S}: minimum {k} against naf_chain_path_check: "
              f"{'bit-equal' if np.array_equal(bits(out[:, k]), bits(out8[:, k])) else f'{err:.2e}'} (tol {tol:.2e})")
        assert err <= tol, (k, err, tol)
    clean = ~P.band_of(case, P.margins_at(case, poses.reshape(N, Cn, S, -1))).any(axis=-1).reshape(N * Cn)
    assert np.array_equal(out[clean][:, [3, 4, 7]], out8[clean][:, [3, 4, 7]])


def test_boxes_without_pairs_through_the_kernel():
    """chain_cert_common.boxes_without_pairs: iiwa_like7 without self-collision among its boxes launches the one-wave CELL + BOX
    instantiation, which no arm of chain_path_common does. The same teacher-forced checks, and parity with naf_chain_path_check."""
    case = K.boxes_without_pairs()
    rig = CertRig(case)
    out, poses = rig.run()
    rig.close()
    old = PathRig(case)
    out8, _ = old.run()
    old.close()
    census = K.check_records(case, out, poses)
    assert census["certified"] >= 1 and np.all(np.isposinf(out[:, 9])) and np.all(np.isfinite(out[:, 10]))
    assert np.array_equal(bits(out[:, 5]), bits(out8[:, 5])) and np.array_equal(out[:, [3, 4, 7]], out8[:, [3, 4, 7]])
    assert np.abs(out[:, [0, 2]].astype(np.float64) - out8[:, [0, 2]]).max() <= C.tol_of(case.model)


def test_the_missed_contact_through_the_kernel():
    """chain_cert_common.missed_contact on the device: the sampled part of the record says free, the certificate names a sample, and
    the obstacle's slack is the twin's to within the band."""
    case, orad = K.missed_contact()
    rig = CertRig(case, orad)
    out, _ = rig.run()
    rig.close()
    want = certify_joint_path(case.twin, case.q_start[0], case.vias[0, 0], case.q_goal[0], case.obstacles[0], case.S, case.margin)
    rec = out[0]
    print(f"device {rec.tolist()}\ntwin   {want.tolist()}")
    assert rec[4] == 0 and rec[3] == -1 and rec[7] == 0 and rec[6] >= 0.05
    assert rec[11] >= 0 and rec[8] < case.margin
    assert abs(float(rec[8]) - want[8]) <= float(K.bounds_of(case)[0, 0, 0]) + 2 * P.POSE_BOUND * case.model.reach
    assert rec[11] == want[11]


def test_refusals_launch_nothing():
    """Every NAF_ERR_ARG case on a real handle: the return code, and the poisoned record stays poisoned."""
    rig = CertRig(P.build_case("iiwa_like7", 1, 1, 64))
    for kw in (dict(h=None), dict(a=None), dict(b=None), dict(v=None), dict(o=None), dict(out=None), dict(reach=None), dict(N=0),
               dict(N=-2), dict(Cn=0), dict(Cn=65), dict(S=0), dict(S=32), dict(S=96), dict(S=2112), dict(S=-64),
               dict(margin=float("nan")), dict(margin=float("inf")), dict(rad=float("nan")), dict(rad=float("inf")), dict(rad=-0.01),
               dict(N=1 << 29, Cn=4), dict(guard=-1e-6), dict(guard=float("nan")), dict(guard=float("inf"))):
        assert rig.call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.isnan(rig.out).all() and torch.isnan(rig.poses).all()
    out, _ = rig.run()
    rig.close()
    assert np.all(np.isfinite(out[:, [0, 3, 4, 5, 6, 7, 8, 11]]))


def refinement_queries():
    """16 queries on iiwa_like7 among its boxes: free start poses; the goals of the first eight a short move away (they certify at
    64 samples or are blocked at an end pose), those of the others up to 2.4 rad per joint (the twin takes one to five rounds over
    them); every fourth obstacle on the straight line's middle"""
    model, twin = P.arm("iiwa_like7")
    rng = np.random.default_rng(52)
    N = 16
    q = P.IK.free_poses(model, twin, rng, N)
    lo, hi = C.limits_of(model)
    span = np.where(np.arange(N) < 8, 0.8, 2.4)[:, None]
    a, b = C.f32(q), C.f32(np.clip(q + rng.uniform(-1.0, 1.0, q.shape) * span, lo, hi))
    ob = C.f32(np.tile(C.away(model)[1], (N, 1)))
    ob[::4] = C.f32(twin.end_effector(0.5 * (a + b)))[::4]
    return model, twin, a, b, ob


def test_refinement_end_to_end_against_the_twin():
    """JointPathChecker(certify=True) against joint_paths_host(certify=True): 16 queries x 8 candidates from 64 samples (resolution
    1 rad). The device's slacks lie within w = 4 tol + 2^-20 beta of the twin's, so every verdict of every round lies between the
    twin's at margin - w and margin + w: a query on which those two twin runs agree has no decisive slack inside a band, and there
    outcome, candidate, certified, samples and refinements equal the twin's at the margin and certified_slack is within w. At least
    half of the queries are such, and some were refined."""
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    model, twin, a, b, ob = refinement_queries()
    margin = P.MARGINS["iiwa_like7"]
    w = 4 * C.tol_of(model) + 2.0 ** -20 * 0.25 + 2 * P.POSE_BOUND * model.reach
    kw = dict(candidates=8, resolution=1.0, seed=9)
    dev = JointPathChecker(model, P.ORAD, certify=True).check(a, b, ob, margin=margin, **kw)
    host, below, above = (joint_paths_host(twin, a, b, ob, margin=float(np.float32(margin)) + d, certify=True, **kw) for d in (0.0, -w, w))
    names = ("outcome", "candidate", "certified", "samples", "refinements")
    sure = np.all([getattr(below, f) == getattr(above, f) for f in names], axis=0)
    print(f"outcomes {dict(zip(*np.unique(dev.outcome, return_counts=True)))}, refinements {dev.refinements.tolist()}, "
          f"{int(sure.sum())} of {len(sure)} queries sure")
    assert sure.sum() >= len(sure) // 2 and dev.refinements.max() >= 1 and dev.certified.any()
    for f in names:
        assert np.array_equal(getattr(dev, f)[sure], getattr(host, f)[sure]), f
    assert dev.certified_slack.dtype == np.float32 and dev.certified.dtype == bool and dev.refinements.dtype == np.int64
    both = sure & np.isfinite(host.certified_slack)
    assert np.all(np.abs(dev.certified_slack[both].astype(np.float64) - host.certified_slack[both]) <= w)
    assert np.array_equal(dev.certified, np.isin(dev.outcome, ("straight", "via")))


def test_framework_certify_and_off_means_off(monkeypatch):
    """plan_joint_paths(certify=True) on the device is JointPathChecker(certify=True) of the same queries, the new fields filled.
    Without the argument the result equals the JointPathChecker of today field for field, nothing is certified, and
    naf_chain_path_certify is not called."""
    from robotic_manipulator_rloa_amd import ManipulatorFramework, _lib
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(**IIWA_RANGED)
    env = f.env
    rng = np.random.default_rng(8)
    goals = P.IK.free_poses(env.model, env, rng, 12)
    start = np.tile(env.initial_joint_positions, (12, 1))
    ob = np.tile(env.obstacle_centre if env.scene_ranges_on else env.obstacle_pos, (12, 1))
    kw = dict(candidates=8, resolution=0.05, seed=3)
    got = f.plan_joint_paths(goal_joint_positions=goals, certify=True, **kw)
    want = JointPathChecker(env.model, env.obstacle_radius, certify=True).check(start, goals, ob, **kw)
    assert isinstance(got, JointPaths)
    for name, x, y in zip(got._fields, got, want):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    assert got.certified.shape == (12,) and got.certified.dtype == bool and got.certified_slack.dtype == np.float32
    assert np.array_equal(got.certified, np.isin(got.outcome, ("straight", "via"))) and got.certified.any()
    assert np.all(got.certified_slack[got.certified] >= 0.0) and np.all(got.refinements >= 0)

    def boom(*args):
        raise AssertionError("naf_chain_path_certify was called without certify")
    monkeypatch.setattr(_lib.load(), "naf_chain_path_certify", boom)
    plain = f.plan_joint_paths(goal_joint_positions=goals, **kw)
    today = JointPathChecker(env.model, env.obstacle_radius).check(start, goals, ob, **kw)
    for name, x, y in zip(plain._fields, plain, today):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    assert not plain.certified.any() and np.all(np.isnan(plain.certified_slack)) and not plain.refinements.any()
    # plain and certified calls alternate without rebuilding either checker
    tools = f.arm_planner.tools                  # kind -> (key, tool)
    kept = (tools["paths"][1], tools["certified_paths"][1])
    assert kept[0] is not kept[1]
    monkeypatch.undo()
    again = f.plan_joint_paths(goal_joint_positions=goals, certify=True, **kw)
    f.plan_joint_paths(goal_joint_positions=goals, **kw)
    assert (tools["paths"][1], tools["certified_paths"][1]) == kept and again.outcome.tobytes() == got.outcome.tobytes()
    assert np.all(np.isin(plain.outcome, ("straight", "via", "blocked", "start", "goal")))
