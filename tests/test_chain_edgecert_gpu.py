"""GPU (`-m gpu`): naf_chain_edge_certify (csrc/chain_env.hip) against the float64 rule of environment/edge_certificate.py
(edge_half_steps, certify_joint_edge) and against naf_chain_edge_check on the same inputs, through the C ABI;
chain_certify.PolylineCertifier and ManipulatorFramework.certify_joint_paths against certify_polylines_host; and that a session which
never asks for a certificate never launches one. tests/test_chain_edgecert_cpu.py rehearses every case with a float32 restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_edgecert_common as E
import chain_roadmap_common as R
import chain_rollout_common as C
from test_chain_edgecert_cpu import EXTRA_ERRORS
from test_chain_roadmap_cpu import ARGUMENT_ERRORS
from test_chain_roadmap_gpu import PAD, EdgeRig, bits
from test_chain_rollout_gpu import IIWA_RANGED

from robotic_manipulator_rloa_amd.environment.edge_certificate import PathCertificates, certify_joint_edge, certify_polylines_host
from robotic_manipulator_rloa_amd.environment.kinematic import certificate_guard, reach_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


class EdgeCertRig:
    """The certifying edge launch of one case through the C ABI; out and poses_out have PAD poisoned items behind the launch's."""

    def __init__(self, case, orad=R.ORAD):
        from robotic_manipulator_rloa_amd import _lib
        self.lib, self.case, self.orad = _lib.load(), case, float(np.float32(orad))
        model = case.model
        self.K, self.S, self.A = case.N * case.E, case.S, model.A
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)      # noqa: E731
        self.nodes, self.obstacles = dev(case.nodes), dev(case.obstacles)
        self.edges = torch.from_numpy(np.ascontiguousarray(case.edges, np.int32)).to(DEV)
        self.reach, self.guard = dev(reach_table(model)), certificate_guard(model)
        nan = dict(fill_value=float("nan"), device=DEV)
        self.out = torch.full((self.K + PAD, 12), **nan)
        self.poses = torch.full((self.K + PAD, self.S, self.A), **nan)

    def call(self, poses=True, **over):
        """the entry point's return code, with the case's arguments but for `over`"""
        p = lambda t: t.data_ptr()      # noqa: E731
        case = self.case
        a = dict(h=self.h, nodes=p(self.nodes), edges=p(self.edges), o=p(self.obstacles), rad=self.orad, reach=p(self.reach),
                 guard=self.guard, N=case.N, V=case.V, E=case.E, S=case.S, margin=case.margin, out=p(self.out))
        a.update(over)
        return self.lib.naf_chain_edge_certify(a["h"], a["nodes"], a["edges"], a["o"], a["rad"], a["reach"], a["guard"], a["N"], a["V"],
                                               a["E"], a["S"], a["margin"], a["out"], p(self.poses) if poses else None,
                                               torch.cuda.current_stream().cuda_stream)

    def run(self, poses=True):
        """returns (out[N E, 12], poses[N E, S, A]) as numpy copies"""
        self.out.fill_(float("nan"))
        assert self.call(poses) == 0
        torch.cuda.synchronize()
        assert torch.isnan(self.out[self.K:]).all() and torch.isnan(self.poses[self.K:]).all()
        return self.out[:self.K].cpu().numpy(), self.poses[:self.K].cpu().numpy()

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


@pytest.mark.parametrize("name,N,V,S", E.CASES)
def test_edge_certify_against_the_rule_and_the_sampled_check(name, N, V, S):
    """One case through the C ABI, poses_out on (the case is the one the CPU rehearsal verified with the twin; the cap and the floors
    are asserted again here, at the recorded poses). Teacher-forced (chain_edgecert_common.check_records): [0 .. 7] pass
    chain_roadmap_common.check_records; the twin's slacks AT THE RECORDED POSES give [8] [9] [10] within 2 tol / 4 tol / 2 tol +
    2^-20 beta and [11] wherever no sample lies inside a band; a case of 64 edges or more holds certified, blocked and
    free-yet-uncertified edges. Parity with naf_chain_edge_check on the same inputs: [5] [6] [7] bit-equal, the three minima within
    1 tol, [3] [4] equal for every edge none of whose samples lies inside a band. A run without poses_out gives the same bits; the
    PAD rows keep their poison. The six arms between them launch all six instantiations."""
    case = E.build(name, N, V, S, verify=False)
    rig = EdgeCertRig(case)
    out, poses = rig.run()
    plain, _ = rig.run(poses=False)
    rig.close()
    old = EdgeRig(case)
    out8, poses8 = old.run()
    old.close()
    assert np.array_equal(bits(out), bits(plain))
    E.check_records(case, out, poses)
    print(f"{name} N={N} V={V} S={S}: poses {'bit-equal' if np.array_equal(bits(poses), bits(poses8)) else 'differ'}")
    assert np.array_equal(bits(out[:, 5:8]), bits(out8[:, 5:8]))
    tol = C.tol_of(case.model)
    for k in range(3):
        got, want = out[:, k].astype(np.float64), out8[:, k].astype(np.float64)
        both_inf = np.isposinf(got) & np.isposinf(want)
        err = float(np.abs(np.where(both_inf, 0.0, got) - np.where(both_inf, 0.0, want)).max())
        print(f"{name} N={N} V={V} S={S}: minimum {k} against naf_chain_edge_check: "
              f"{'bit-equal' if np.array_equal(bits(out[:, k]), bits(out8[:, k])) else f'{err:.2e}'} (tol {tol:.2e})")
        assert err <= tol, (k, err, tol)
    clean = ~R.band_of(case, R.margins_at(case, poses.reshape(N, case.E, S, -1))).any(axis=-1).reshape(N * case.E)
    assert np.array_equal(out[clean][:, [3, 4]], out8[clean][:, [3, 4]])


def test_the_missed_contact_through_the_kernel():
    """chain_edgecert_common.missed_contact on the device: the sampled part of the record says free, the certificate names a sample,
    and the obstacle's slack is the twin's to within the band."""
    case, orad = E.missed_contact()
    rig = EdgeCertRig(case, orad)
    out, _ = rig.run()
    rig.close()
    want = certify_joint_edge(case.twin, case.nodes[0, 0], case.nodes[0, 1], case.obstacles[0], case.S, case.margin)
    rec = out[0]
    print(f"device {rec.tolist()}\ntwin   {want.tolist()}")
    assert rec[4] == 0 and rec[3] == -1 and rec[7] == 0 and rec[6] >= 0.05
    assert rec[11] >= 0 and rec[8] < case.margin
    assert abs(float(rec[8]) - want[8]) <= float(E.bounds_of(case)[0, 0, 0]) + 2 * R.POSE_BOUND * case.model.reach
    assert rec[11] == want[11]


def test_refusals_launch_nothing():
    """Every NAF_ERR_ARG case on a real handle — naf_chain_edge_check's list, and a null reach and a negative or non-finite guard:
    the return code, and the poisoned buffers stay poisoned. (No arm of the suite is accepted by naf_chain_env_create and then too
    large for the table: NAF_CHAIN_ERR_LDS is not run here; the CPU suite holds the facade's answer to it.)"""
    rig = EdgeCertRig(R.build_case("planar3", 3, 5, 128, verify=False))
    for kw in ARGUMENT_ERRORS + EXTRA_ERRORS:                                # (stated against one query of one edge, as the CPU suite's)
        assert rig.call(**{**dict(N=1, V=2, E=1, S=64), **kw}) == -1, kw
    torch.cuda.synchronize()
    assert torch.isnan(rig.out).all() and torch.isnan(rig.poses).all()
    out, _ = rig.run()
    rig.close()
    assert not np.isnan(out).any()


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
NAMES = ("outcome", "samples", "refinements", "weakest_leg")


@pytest.mark.parametrize("shortcut", [0, E.SHORTCUT])
def test_polyline_certifier_end_to_end_against_the_twin(shortcut):
    """PolylineCertifier.certify against certify_polylines_host on the 24-query iiwa_like7 set (roadmap=14), without and with
    shortcut=16, at the resolution the set was planned with. The device's slacks lie within w = 4 tol + 2^-20 beta + 2 POSE_BOUND
    reach of the twin's, so every verdict of every round lies between the twin's at margin - w and margin + w
    (test_refinement_end_to_end_against_the_twin's band method): on the queries where those two twin runs agree, outcome, samples,
    refinements and weakest_leg equal the twin's at the margin and slack is within w. At least half of the queries are such, and at
    least one was refined."""
    from robotic_manipulator_rloa_amd.chain_certify import PolylineCertifier
    model, twin = R.arm("iiwa_like7")
    paths, ob, margin = E.polyline_paths("iiwa_like7", shortcut, R.IIWA_CUT)
    res = R.VALUE_KW["resolution"]
    w = 4 * C.tol_of(model) + 2.0 ** -20 * 0.25 + 2 * R.POSE_BOUND * model.reach
    tool = PolylineCertifier(model, R.ORAD)
    dev = tool.certify(paths, ob, margin, res)
    host, below, above = (certify_polylines_host(twin, paths, ob, float(np.float32(margin)) + d, res) for d in (0.0, -w, w))
    sure = np.all([getattr(below, f) == getattr(above, f) for f in NAMES], axis=0)
    print(f"shortcut {shortcut}: outcomes {dict(zip(*np.unique(dev.outcome, return_counts=True)))}, refinements {dev.refinements.tolist()}, "
          f"{int(sure.sum())} of {len(sure)} queries sure, {tool.launches} launches")
    assert isinstance(dev, PathCertificates) and sure.sum() >= len(sure) // 2 and dev.refinements.max() >= 1 and dev.certified.any()
    for f in NAMES:
        assert np.array_equal(getattr(dev, f)[sure], getattr(host, f)[sure]), f
    assert dev.slack.dtype == np.float32 and dev.leg_slack.dtype == np.float32 and dev.certified.dtype == bool
    assert dev.refinements.dtype == np.int64 and dev.samples.dtype == np.int64 and dev.leg_slack.shape == host.leg_slack.shape
    both = sure & np.isfinite(host.slack)
    assert np.all(np.abs(dev.slack[both].astype(np.float64) - host.slack[both]) <= w)
    assert np.array_equal(dev.outcome == "none", host.outcome == "none") and np.array_equal(dev.certified, dev.outcome == "certified")
    with pytest.raises(ValueError, match="exceed the chunk"):
        PolylineCertifier(model, R.ORAD, chunk=64).certify(paths, ob, margin, res)


# ---- the façade ----------------------------------------------------------------------------------------------------------------------
def test_framework_certify_joint_paths_and_off_means_off(monkeypatch, scratch_cwd):
    """certify_joint_paths on the device equals PolylineCertifier of the same paths byte for byte; a second call reuses the cached
    tool; plan_joint_paths' results and the training-state digest are what they are without the call; and a session that never
    calls the method never calls naf_chain_edge_certify (monkeypatched to raise)."""
    from chain_resume_worker import make_framework
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_certify import PolylineCertifier
    f = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    env = f.env
    before = f.naf_agent.training_state_digest()
    rng = np.random.default_rng(8)
    N = 12
    goals = R.IK.free_poses(env.model, env, rng, N)
    start = np.tile(env.initial_joint_positions, (N, 1))
    ob = np.tile(env.obstacle_centre if env.scene_ranges_on else env.obstacle_pos, (N, 1)).astype(np.float64)
    ob[1::2] = env.end_effector(0.5 * (start + goals))[1::2]
    kw = dict(goal_joint_positions=goals, obstacles=ob, candidates=1, resolution=0.05, seed=3, roadmap=R.ROADMAP, shortcut=E.SHORTCUT)
    paths = f.plan_joint_paths(**kw)
    assert "polyline_certificates" not in f.arm_planner.tools
    got = f.certify_joint_paths(paths, obstacles=ob, clearance_margin=0.002, resolution=0.05)
    tool = f.arm_planner.tools["polyline_certificates"][1]
    want = PolylineCertifier(env.model, env.obstacle_radius).certify(paths, ob, 0.002, 0.05)
    print({o: int(np.sum(got.outcome == o)) for o in sorted(set(got.outcome))}, "of", {o: int(np.sum(paths.outcome == o)) for o in sorted(set(paths.outcome))})
    for name, x, y in zip(got._fields, got, want):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    assert got.certified.any() and np.array_equal(got.outcome == "none", (paths.candidate < 0) & (paths.n_nodes < 2))
    again = f.certify_joint_paths(paths, obstacles=ob, clearance_margin=0.002, resolution=0.05)
    assert f.arm_planner.tools["polyline_certificates"][1] is tool and again.outcome.tobytes() == got.outcome.tobytes()
    assert f.naf_agent.training_state_digest() == before
    replanned = f.plan_joint_paths(**kw)
    for name, x, y in zip(paths._fields, replanned, paths):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    assert replanned.nodes.tobytes() == paths.nodes.tobytes() and replanned.n_nodes.tobytes() == paths.n_nodes.tobytes()

    def boom(*args):
        raise AssertionError("naf_chain_edge_certify was called without certify_joint_paths")
    monkeypatch.setattr(_lib.load(), "naf_chain_edge_certify", boom)
    g = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    fresh = g.naf_agent.training_state_digest()
    quiet = g.plan_joint_paths(**kw)
    g.demonstrate_joint_paths(quiet, obstacles=ob, polylines=True)
    assert quiet.outcome.tobytes() == paths.outcome.tobytes() and "polyline_certificates" not in g.arm_planner.tools
    assert g.naf_agent.training_state_digest() == fresh
