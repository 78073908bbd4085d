"""GPU (`-m gpu`): naf_chain_edge_check (csrc/chain_env.hip) against the float64 rule of environment/kinematic.py (edge_pose,
check_joint_edge) through the C ABI; chain_tools.JointPathChecker.check(roadmap=M), ManipulatorFramework.plan_joint_paths(roadmap=M) and
reach_targets(joint_paths=True, roadmap=M) against that rule and roadmap_search; and that training launches are untouched.
tests/test_chain_roadmap_cpu.py rehearses every case with a float32 restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_roadmap_common as R
import chain_rollout_common as C
from test_chain_env_gpu import _agent
from test_chain_roadmap_cpu import ARGUMENT_ERRORS
from test_chain_rollout_gpu import IIWA_RANGED, _training_stream_digest

from robotic_manipulator_rloa_amd.environment import kinematic as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 5                        # items behind the N E of the launch that no lane may write
GATHER = K.gather_roadmap_paths


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class EdgeRig:
    """The edge launch of one case through the C ABI; out and poses_out have PAD poisoned items behind the launch's."""

    def __init__(self, case):
        from robotic_manipulator_rloa_amd import _lib
        self.lib = _lib.load()
        self.case = case
        model = case.model
        self.K, self.S, self.A = case.N * case.E, case.S, model.A
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)      # noqa: E731
        self.nodes, self.obstacles = dev(case.nodes), dev(case.obstacles)
        self.edges = torch.from_numpy(np.ascontiguousarray(case.edges, np.int32)).to(DEV)
        nan = dict(fill_value=float("nan"), device=DEV)
        self.out = torch.full((self.K + PAD, 8), **nan)
        self.poses = torch.full((self.K + PAD, self.S, self.A), **nan)

    def call(self, poses=True, stream=None, **over):
        """the entry point's return code, with the case's arguments but for `over`"""
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        p = lambda t: t.data_ptr()      # noqa: E731
        case = self.case
        a = dict(h=self.h, nodes=p(self.nodes), edges=p(self.edges), o=p(self.obstacles), rad=R.ORAD, N=case.N, V=case.V, E=case.E,
                 S=case.S, margin=case.margin, out=p(self.out))
        a.update(over)
        return self.lib.naf_chain_edge_check(a["h"], a["nodes"], a["edges"], a["o"], a["rad"], a["N"], a["V"], a["E"], a["S"],
                                             a["margin"], a["out"], p(self.poses) if poses else None, st)

    def run(self, poses=True, stream=None):
        """returns (out[N E, 8], poses[N E, S, A]) as numpy copies"""
        self.out.fill_(float("nan"))
        assert self.call(poses, stream) == 0
        torch.cuda.synchronize()
        assert torch.isnan(self.out[self.K:]).all() and torch.isnan(self.poses[self.K:]).all()
        return self.out[:self.K].cpu().numpy(), self.poses[:self.K].cpu().numpy()

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


CASES = [(name, N, V, S) for name in R.ARMS for N, V, S in R.COUNTS] + R.EXTRA


@pytest.mark.parametrize("name,N,V,S", CASES)
def test_edge_check_against_the_rule(name, N, V, S):
    """One case through the C ABI, poses_out on (the case is the one the CPU rehearsal verified with the twin; the cap and the
    floors are asserted again here, at the recorded poses). Teacher-forced: every recorded pose within
    chain_roadmap_common.POSE_BOUND (8 x the float32 restatement's measured deviation) of edge_pose; the twin AT THE RECORDED POSES
    gives the three minima within 2 tol / 4 tol / 2 tol (+inf where the model has no pairs / no workcell), [5] bit for bit, [6]
    within an ulp, [7] zero, and [3], [4] wherever no sample lies inside a band, bracketed by the sure and the possible samples
    otherwise (chain_roadmap_common.check_records). A run without poses_out gives the same bits, and the PAD rows keep their
    poison. The six arms between them launch all six instantiations."""
    case = R.build_case(name, N, V, S, verify=False)
    rig = EdgeRig(case)
    out, poses = rig.run()
    plain, _ = rig.run(poses=False)
    rig.close()
    assert np.array_equal(bits(out), bits(plain))
    R.check_records(case, out, poses)


def test_placement_independence_and_a_permuted_edge_list():
    """Edge (3, 9) of query 5 of the 8 x 16 case gives the same eight floats and the same poses alone — a launch of one query with
    that one edge — as deep inside the launch of 960; the whole launch under a permuted edges_dev gives every record at its
    permuted place, bit for bit; a launch on a side stream gives the current stream's bits."""
    case = R.build_case("iiwa_like7", 8, 16, 256, verify=False)
    rig = EdgeRig(case)
    big, big_poses = rig.run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side, _ = rig.run(stream=side.cuda_stream)
    rig.close()
    assert np.array_equal(bits(big), bits(on_side))
    n, e = 5, int(np.nonzero((case.edges[:, 0] == 3) & (case.edges[:, 1] == 9))[0][0])
    one = EdgeRig(case.sub(n, [(3, 9)]))
    alone, alone_poses = one.run()
    one.close()
    assert np.array_equal(bits(big[n * case.E + e]), bits(alone[0])) and np.array_equal(bits(big_poses[n * case.E + e]), bits(alone_poses[0]))
    perm = np.random.default_rng(4).permutation(case.E)
    shuffled = EdgeRig(R.Case(case.name, case.N, case.V, case.S, case.nodes, case.obstacles, case.margin, case.edges[perm]))
    out, _ = shuffled.run(poses=False)
    shuffled.close()
    assert np.array_equal(bits(out.reshape(case.N, case.E, 8)), bits(big.reshape(case.N, case.E, 8)[:, perm]))
    some = EdgeRig(case.sub(n, case.edges[perm[:7]]))                       # a subset of the edges: E = 7 of the 120
    part, _ = some.run(poses=False)
    some.close()
    assert np.array_equal(bits(part), bits(big.reshape(case.N, case.E, 8)[n, perm[:7]]))


def test_argument_errors_launch_nothing():
    """Every refusal include/naf_hip.h names returns NAF_ERR_ARG with a real handle and real buffers, and the poisoned record buffer
    is still poisoned behind them all: nothing was launched."""
    case = R.build_case("planar3", 3, 5, 128, verify=False)
    rig = EdgeRig(case)
    rig.out.fill_(float("nan"))
    for kw in ARGUMENT_ERRORS:                                              # (stated against one query of one edge, as the CPU suite's)
        assert rig.call(**{**dict(N=1, V=2, E=1, S=64), **kw}) == -1, kw
    torch.cuda.synchronize()
    assert torch.isnan(rig.out).all()
    out, _ = rig.run()
    assert not np.isnan(out).any()
    rig.close()


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def checked_with_records(monkeypatch, name, cut=None, chunk=None):
    """JointPathChecker.check(roadmap=14) on a value set, without and with the roadmap, and what the roadmap round gathered from"""
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    q0, q1, ob, margin = R.value_queries(name, cut)
    seen = {}
    gather = GATHER

    def recording(base, blocked, records, nodes, edges, samples):
        seen.update(blocked=np.array(blocked), records=np.array(records), nodes=np.array(nodes), edges=np.array(edges),
                    samples=np.array(samples))
        return gather(base, blocked, records, nodes, edges, samples)

    monkeypatch.setattr(K, "gather_roadmap_paths", recording)
    checker = JointPathChecker(R.arm(name)[0], R.ORAD, **({} if chunk is None else dict(chunk=chunk)))
    kw = dict(margin=margin, **R.VALUE_KW)
    base = checker.check(q0, q1, ob, **kw)
    assert checker.edge_launches == 0 and checker.edge_nodes is None and base.nodes is None
    out = checker.check(q0, q1, ob, roadmap=R.ROADMAP, **kw)
    return checker, base, out, seen, (q0, q1, ob, margin)


@pytest.mark.parametrize("name,cut", [("planar3", None), ("iiwa_like7", R.IIWA_CUT)])
def test_joint_path_checker_with_a_roadmap_end_to_end(monkeypatch, name, cut):
    """JointPathChecker.check(roadmap=14) on the value test's planar3 set and on the 24-query cut of its iiwa_like7 set (which the
    CPU suite's twin shows holds at least 2 rescued queries): roadmap_search applied to the device's own records reproduces nodes,
    n_nodes and length bit for bit; every returned edge is free at the twin's sure samples; every query that was not 'blocked' is
    bit-equal to the call without roadmap; at least one query ends 'roadmap'; the records are float32 and their nodes the rule's."""
    checker, base, out, seen, (q0, q1, ob, margin) = checked_with_records(monkeypatch, name, cut)
    N, V = len(q0), R.ROADMAP + 2
    blocked = np.nonzero(base.outcome == "blocked")[0]
    assert np.array_equal(seen["blocked"], blocked) and seen["records"].dtype == np.float32
    assert seen["records"].shape == (len(blocked), V * (V - 1) // 2, 8) and np.array_equal(seen["edges"], K.roadmap_edges(V))
    want_nodes = K.roadmap_nodes(q0, q1, K.roadmap_milestones(checker.chain, q0, q1, R.ROADMAP, R.VALUE_KW["seed"]))
    assert np.array_equal(bits(seen["nodes"]), bits(want_nodes[blocked])) and checker.edge_launches >= 1
    n_nodes, index, length = K.roadmap_search(seen["records"], seen["edges"], V)
    rescued = out.outcome == "roadmap"
    print(name, {o: int(np.sum(out.outcome == o)) for o in sorted(set(out.outcome))}, "from", int(len(blocked)), "blocked")
    assert rescued.sum() >= 1 and np.array_equal(np.nonzero(rescued)[0], blocked[n_nodes > 0])
    assert np.array_equal(out.n_nodes[blocked], n_nodes) and np.all(out.n_nodes[base.outcome != "blocked"] == 0)
    assert out.nodes.dtype == np.float32 and out.nodes.shape == (N, n_nodes.max(), q0.shape[1]) and out.length.dtype == np.float32
    for k, q in enumerate(blocked):
        if n_nodes[k]:
            assert np.array_equal(bits(out.nodes[q, :n_nodes[k]]), bits(seen["nodes"][k, index[k, :n_nodes[k]]]))
            assert np.all(np.isnan(out.nodes[q, n_nodes[k]:])) and bits(out.length[q]) == bits(length[k])
            assert out.samples[q] == seen["samples"][k] and out.candidate[q] == -1 and np.all(np.isnan(out.via[q]))
    assert np.array_equal(out.roadmap_free_edges[blocked], np.sum(seen["records"][..., 4] == 0, axis=1))
    assert np.all(out.roadmap_free_edges[base.outcome != "blocked"] == -1)
    for field, x, y in zip(base._fields, out, base):
        assert x.dtype == y.dtype and x[~rescued].tobytes() == y[~rescued].tobytes(), field
    assert R.edges_free_at_sure_samples(name, out, ob, margin) == int((out.n_nodes[rescued] - 1).sum())


def test_joint_path_checker_roadmap_chunks_and_refusals(monkeypatch):
    """A budget that holds one query's 120 edges at a time gives the fields of the single chunk wherever both sample alike (the
    chunk's S is its own queries'), the launches counted; refusals of check()."""
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    _, _, whole, seen, (q0, q1, ob, margin) = checked_with_records(monkeypatch, "planar3")
    E = len(seen["edges"])
    small, _, parts, seen_parts, _ = checked_with_records(monkeypatch, "planar3", chunk=E * int(seen["samples"].max()))
    assert small.edge_launches == len(seen["blocked"]) >= 2
    alike = seen_parts["samples"] == seen["samples"]
    assert alike.any() and np.array_equal(bits(seen_parts["records"][alike]), bits(seen["records"][alike]))
    with pytest.raises(ValueError, match="roadmap is a number of milestones from 0 to 62"):
        small.check(q0, q1, ob, roadmap=63)
    with pytest.raises(ValueError, match="exceed the chunk"):
        JointPathChecker(R.arm("planar3")[0], R.ORAD, chunk=16 * 64).check(q0, q1, ob, margin=margin, roadmap=R.ROADMAP, **R.VALUE_KW)
    with pytest.raises(ValueError, match="0 <= i < j < 4"):
        small.load_edges(np.zeros((1, 4, 3), np.float32), [[0, 1], [2, 4]], np.zeros((1, 3)))
    with pytest.raises(ValueError, match="0 <= i < j < 4"):
        small.load_edges(np.zeros((1, 4, 3), np.float32), [[1, 1]], np.zeros((1, 3)))


# ---- the façade ----------------------------------------------------------------------------------------------------------------------
def test_framework_roadmap_end_to_end(scratch_cwd):
    """plan_joint_paths(roadmap=14) and reach_targets(joint_paths=True, roadmap=14) on a freshly initialised agent: the fields have
    the stated shapes, every query that is not 'roadmap' is bit-equal to the call without the argument, planned_ratio is finite
    for a reached 'roadmap' query (if there is one) and NaN where there is no path; the rollout's numbers are the plain call's; no
    call changes the training-state digest; roadmap with certify is refused."""
    from chain_resume_worker import make_framework
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    N, F, A = 24, 20, 7
    rng = np.random.default_rng(8)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.15, 0.15, (N, 3))
    targets[-1] = [0.0, 0.0, 2.0]                                      # out of reach
    # the obstacle of every second query sits where the straight line to a goal pose passes: few candidates, so that some are blocked
    f = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    before = f.naf_agent.training_state_digest()
    goal = f.solve_goal_poses(targets, seed=3)
    start = np.tile(f.env.initial_joint_positions, (N, 1))
    obstacles = np.tile(f.env.obstacle_centre if f.env.scene_ranges_on else f.env.obstacle_pos, (N, 1)).astype(np.float64)
    mid = f.env.end_effector(0.5 * (start + np.asarray(goal.joint_positions, np.float64)))
    obstacles[1::2] = np.where(np.asarray(goal.reachable)[1::2, None], mid[1::2], obstacles[1::2])
    kw = dict(obstacles=obstacles, candidates=2, seed=3, resolution=0.05)
    plain = f.plan_joint_paths(targets, **kw)
    out = f.plan_joint_paths(targets, roadmap=R.ROADMAP, **kw)
    assert f.naf_agent.training_state_digest() == before
    print({o: int(np.sum(plain.outcome == o)) for o in sorted(set(plain.outcome))}, "->",
          {o: int(np.sum(out.outcome == o)) for o in sorted(set(out.outcome))})
    assert plain.nodes is None and plain.n_nodes is None and plain.roadmap_free_edges is None
    rescued = out.outcome == "roadmap"
    assert np.all(plain.outcome[rescued] == "blocked")
    for field, x, y in zip(plain._fields, out, plain):
        assert x.dtype == y.dtype and x.shape == y.shape and x[~rescued].tobytes() == y[~rescued].tobytes(), field
    K_nodes = int(out.n_nodes.max())
    assert out.nodes.shape == (N, K_nodes, A) and out.n_nodes.shape == (N,) and out.roadmap_free_edges.shape == (N,)
    assert np.array_equal(out.n_nodes > 0, rescued) and np.array_equal(out.roadmap_free_edges >= 0, plain.outcome == "blocked")
    assert out.outcome[-1] == "goal" and out.n_nodes[-1] == 0 and np.all(np.isnan(out.nodes[-1]))
    assert np.all(np.isfinite(out.length[rescued])) and np.all(out.candidate[rescued] == -1)
    assert out.waypoints(7).shape == (N, 7, A) and not np.any(np.isnan(out.waypoints(7)[rescued]))
    demos = f.demonstrate_joint_paths(out, targets)
    assert np.all(demos.outcome[rescued] == "none")
    base = f.reach_targets(targets, obstacles=obstacles, frames=F)
    got = f.reach_targets(targets, obstacles=obstacles, frames=F, joint_paths=True, roadmap=R.ROADMAP)
    assert f.naf_agent.training_state_digest() == before
    for name in ("outcome", "frames", "final_distance", "min_clearance", "min_self_clearance", "score", "joint_positions",
                 "start_distance", "start_clearance", "start_self_clearance", "min_cell_clearance", "start_cell_clearance"):
        a, b = getattr(got, name), getattr(base, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    default = f.plan_joint_paths(targets, obstacles=obstacles, roadmap=R.ROADMAP)
    for field, x, y in zip(default._fields, got.path, default):
        assert x.tobytes() == y.tobytes(), field
    assert got.path.n_nodes.tobytes() == default.n_nodes.tobytes() and got.path.nodes.tobytes() == default.nodes.tobytes()
    has = np.isfinite(got.path.length.astype(np.float64))
    good = (got.outcome == "reached") & has
    assert got.planned_ratio.shape == (N,) and np.all(np.isnan(got.planned_ratio[~good])) and np.all(np.isfinite(got.planned_ratio[good]))
    assert np.array_equal(has, (got.path.candidate >= 0) | (got.path.outcome == "roadmap"))
    with pytest.raises(InvalidEnvironmentParameter, match="roadmap edges are checked at their samples only"):
        f.plan_joint_paths(targets, roadmap=4, certify=True)
    with pytest.raises(InvalidEnvironmentParameter, match="roadmap is a number of milestones from 0 to 62"):
        f.reach_targets(targets, frames=F, joint_paths=True, roadmap=63)


def test_off_means_off():
    """A fixed-seed DeviceEnvLoop stream (test_chain_rollout_gpu's: 100 steps, E = 64, iiwa_like7 with self-collision) hashes the
    same before and after roadmaps have been checked for the same model in the same process."""
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    model, twin = C.arm("iiwa_like7", True)
    agent = _agent(model)
    before = _training_stream_digest(agent, model, False)
    rng = np.random.default_rng(3)
    N = 32
    q = R.IK.free_poses(model, twin, rng, 2 * N)
    ob = twin.end_effector(0.5 * (q[:N] + q[N:]))
    checker = JointPathChecker(model, R.ORAD)
    out = checker.check(q[:N], q[N:], ob, candidates=1, resolution=0.05, roadmap=6)
    assert checker.edge_launches >= 1 and (out.roadmap_free_edges >= 0).any()
    assert _training_stream_digest(agent, model, False) == before
