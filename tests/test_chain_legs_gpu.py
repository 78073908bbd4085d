"""GPU (`-m gpu`): naf_chain_demo_rows_legs (csrc/chain_env.hip) through the C ABI with poisoned pad rows behind every output —
at K = 2 against naf_chain_demo_rows bit for bit, on the legs cases against the step kernel it restates and the float64 rule of
environment/kinematic.py (demonstration_plan_legs, demo_actions, demonstration_rows_host); placement independence and the refusals;
chain_tools.DemonstrationWriter with K-leg plans; JointPathChecker.check(roadmap=, shortcut=) against roadmap_search on the device's
own records; and plan_joint_paths(shortcut=) -> demonstrate_joint_paths(polylines=True) -> run_training end to end.
tests/test_chain_legs_cpu.py rehearses every case with a float32 restatement."""
import numpy as np
import pytest
import torch

import chain_demo_common as D
import chain_legs_common as L
import chain_roadmap_common as R
import chain_rollout_common as C
from test_chain_demo_gpu import CASES as TWO_LEG_CASES
from test_chain_demo_gpu import PAD, DemoRig, scratch_cwd  # noqa: F401
from test_chain_env_gpu import _agent
from test_chain_legs_cpu import ARGUMENT_ERRORS
from test_chain_rollout_gpu import IIWA_RANGED, _training_stream_digest

from robotic_manipulator_rloa_amd.environment import kinematic as K
from robotic_manipulator_rloa_amd.environment.kinematic import gather_demonstrations

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
bits = D.bits


class LegsRig(DemoRig):
    """test_chain_demo_gpu.DemoRig with the launch of naf_chain_demo_rows_legs: the plan's n_ticks[N][K] and leg_actions[N][K][A] as
    they are; steps(), the composed form, is DemoRig's as it stands (it reads demo_actions)."""

    def call(self, poses=True, stream=None, **over):
        """the entry point's return code, with the case's arguments but for `over`"""
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        p = lambda t: t.data_ptr()      # noqa: E731
        a = dict(h=self.h, q=p(self.q_start), a=p(self.actions), n=p(self.ticks), K=self.ticks.shape[1], t=p(self.targets),
                 o=p(self.obstacles), rad=D.ORAD, N=self.N, T=self.T, rows=p(self.rows), rf=self.rf, rec=p(self.records))
        a.update(over)
        rf = self.rf + 1 if a["rf"] is None else a["rf"]
        return self.lib.naf_chain_demo_rows_legs(a["h"], a["q"], a["a"], a["n"], a["K"], a["t"], a["o"], a["rad"], a["N"], a["T"],
                                                 a["rows"], rf, a["rec"], p(self.poses) if poses else None, st)

    def run(self, poses=True, stream=None):
        for t in (self.rows, self.records, self.poses):
            t.fill_(float("nan"))
        assert self.call(poses, stream) == 0
        torch.cuda.synchronize()
        N = self.N
        assert torch.isnan(self.rows[N:]).all() and torch.isnan(self.records[N:]).all() and torch.isnan(self.poses[N:]).all()
        rows, poses_ = self.rows[:N].cpu().numpy(), self.poses[:N].cpu().numpy()
        Tn = self.case.plan.rows
        assert np.isnan(rows[np.arange(self.T)[None, :] >= Tn[:, None]]).all()             # rows T_n .. T_cap - 1 are not written
        if poses:
            assert np.isnan(poses_[np.arange(self.T + 1)[None, :] > Tn[:, None]]).all()
        return rows, self.records[:N].cpu().numpy(), poses_


class Replanned:
    """a chain_demo_common case under another plan of the same actions: what LegsRig reads of a case"""

    def __init__(self, case, plan):
        self.model, self.N, self.T_cap, self.targets, self.obstacles, self.plan = case.model, case.N, case.T_cap, case.targets, \
            case.obstacles, plan


def same_bits(a, b):
    return all(np.array_equal(bits(np.nan_to_num(x)), bits(np.nan_to_num(y))) and np.array_equal(np.isnan(x), np.isnan(y))
               for x, y in zip(a, b))


# ---- K = 2 is the old kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,T_cap", TWO_LEG_CASES)
def test_two_legs_are_the_two_leg_kernel_bit_for_bit(name, N, T_cap):
    """For every case of test_chain_demo_gpu, rows, records and poses of naf_chain_demo_rows_legs at K = 2 are those of
    naf_chain_demo_rows on the same inputs, NaN poison where nothing is written included; the same with a third, padding leg
    (K = 3, count 0, a poisoned action), and without poses_out."""
    case = D.build_case(name, N, T_cap)
    old = DemoRig(case)
    want = old.run()
    old.close()
    rig = LegsRig(case)
    got, plain = rig.run(), rig.run(poses=False)
    rig.close()
    assert same_bits(got, want) and same_bits(plain[:2], want[:2])
    plan = case.plan
    ticks = np.concatenate([plan.n_ticks, np.zeros((N, 1), np.int32)], axis=1)
    acts = np.concatenate([plan.leg_actions, np.full((N, 1, case.model.A), 7.0, np.float32)], axis=1)
    padded = LegsRig(Replanned(case, plan._replace(n_ticks=ticks, leg_actions=acts)))
    got3 = padded.run()
    padded.close()
    assert same_bits(got3, want)


# ---- the legs cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,K,T_cap", L.CASES)
def test_legs_rows_against_the_step_kernel_and_the_rule(name, N, K, T_cap):
    """One legs case through the C ABI, poses_out on, under the split test_demo_rows_against_the_step_kernel_and_the_rule applies.
    Against the composed form (reset_given, then T_cap x naf_chain_env_step fed demo_actions): for the rows up to each
    demonstration's first done, joint positions, velocities, actions, target, obstacle and the zeros bit for bit; the end effector
    within 1 tol (chain_rollout_common.tol_of); reward class and done equal wherever the twin's margins at the recorded poses lie
    outside the bands (at most 1 % of the ticks inside); the record's count the composed form's first done. Against the float64
    rule and for chain exactness: chain_demo_common.check_rows, and the pose deviation within chain_legs_common.POSE_BOUND. A run
    without poses_out gives the same bits, and the PAD demonstrations and the rows behind T_n keep their poison."""
    case = L.build_case(name, N, K, T_cap)
    rig = LegsRig(case)
    rows, rec, poses = rig.run()
    plain_rows, plain_rec, _ = rig.run(poses=False)
    ref = rig.steps()
    rig.close()
    assert np.array_equal(bits(np.nan_to_num(rows)), bits(np.nan_to_num(plain_rows))) and np.array_equal(bits(rec), bits(plain_rec))
    dev, _, _ = D.check_rows(case, rows, rec, poses)
    print(f"{name} N={N} K={K} T_cap={T_cap}: largest pose deviation {dev:.2e} (bound {L.POSE_BOUND:.2e})")
    assert dev <= L.POSE_BOUND
    A, S, off_s2, off_d = rig.A, rig.S, rig.off_s2, rig.off_d
    tol = C.tol_of(case.model)
    valid = rec[:, 0].astype(np.int64)
    live = np.arange(T_cap)[None, :] < valid[:, None]
    exact = np.zeros(rig.rf, bool)
    for lead in (0, off_s2):
        exact[lead:lead + 2 * A] = True                       # positions and velocities
        exact[lead + 2 * A + 3:lead + 2 * A + 9] = True       # target and obstacle
    exact[S:S + A] = True                                     # the action
    exact[S + A + 1:off_s2] = exact[off_d + 1:] = True        # the zeros, the tag float included
    got, want = rows[live], ref[live]
    assert np.array_equal(bits(got[:, exact]), bits(want[:, exact]))
    in_band = D.band_of(case, D.margins_at(case, np.nan_to_num(poses)))
    band = in_band[live]
    assert band.sum() <= D.CAP * live.sum()
    ee = np.zeros(rig.rf, bool)
    ee[2 * A:2 * A + 3] = ee[off_s2 + 2 * A:off_s2 + 2 * A + 3] = True
    err = float(np.abs(got[:, ee].astype(np.float64) - want[:, ee]).max())
    print(f"{name} N={N} K={K} T_cap={T_cap}: end effector against the step kernel {err:.2e} (tol {tol:.2e}); "
          f"{'every float bit-equal' if np.array_equal(bits(got), bits(want)) else 'not to the bit'}")
    assert err <= tol
    sure = ~band
    assert np.array_equal(got[sure, off_d], want[sure, off_d])
    r_got, r_want = got[sure, S + A].astype(np.float64), want[sure, S + A].astype(np.float64)
    terminal = (r_want == 250.0) | (r_want == -1000.0)
    assert np.array_equal(r_got[terminal], r_want[terminal]) and np.abs(r_got - r_want)[~terminal].max(initial=0.0) <= tol
    first_band = np.array([in_band[n, :valid[n]].any() for n in range(N)])
    ref_done = ref[..., off_d] == 1.0
    ref_valid = np.where(ref_done.any(axis=1), ref_done.argmax(axis=1) + 1, T_cap + 1)
    Tn = case.plan.rows
    assert np.array_equal(valid[~first_band], np.minimum(ref_valid, Tn)[~first_band])
    _, h_rec, _, _ = case.host()
    if not first_band.any():
        assert np.array_equal(rec[:, 0], h_rec[:, 0]) and np.array_equal(rec[:, 1], h_rec[:, 1])
    assert np.array_equal(rec[:, 6], case.plan.n_ticks.sum(axis=1))


# ---- placement and refusals ------------------------------------------------------------------------------------------------------
def test_placement_independence_through_the_c_abi():
    """A demonstration of the 8 x 5-leg x 256 case gives the same rows, record and poses alone at index 0 of a launch of one as
    inside the launch of 8, bit for bit; a launch on a side stream gives the current stream's bits."""
    case = L.build_case("iiwa_like7", 8, 5, 256)
    rig = LegsRig(case)
    big = rig.run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = rig.run(stream=side.cuda_stream)
    rig.close()
    assert same_bits(big, on_side)
    for n in (4, 7):
        one = LegsRig(case.sub(n))
        alone = one.run()
        one.close()
        for a, b in zip(big, alone):
            assert np.array_equal(bits(np.nan_to_num(a[n])), bits(np.nan_to_num(b[0])))


def test_argument_errors_launch_nothing():
    """Every refusal include/naf_hip.h names returns NAF_ERR_ARG with a real handle and real buffers, and the poisoned outputs are
    still poisoned behind them all: nothing was launched."""
    case = L.build_case("planar3", 3, 3, 130)
    rig = LegsRig(case)
    for t in (rig.rows, rig.records, rig.poses):
        t.fill_(float("nan"))
    for kw in ARGUMENT_ERRORS:
        assert rig.call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.isnan(rig.rows).all() and torch.isnan(rig.records).all() and torch.isnan(rig.poses).all()
    _, rec, _ = rig.run()
    assert not np.isnan(rec).any()
    rig.close()


# ---- the writer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,K,T_cap,chunk", [("iiwa_like7", 8, 5, 256, 2 * 256), ("long12", 2, 63, 130, 130),
                                                  ("slider4", 8, 5, 256, None)])
def test_demonstration_writer_with_legs_across_chunks_and_the_ring(name, N, K, T_cap, chunk):
    """chain_tools.DemonstrationWriter with a K-leg plan in forced small chunks and in one chunk gives the kept rows of one C-ABI
    launch, in query order then tick order, and its numbers, through naf_chain_demo_rows_legs alone; after add_demonstrations on a
    fresh agent the ring reads back exactly those rows. A two-leg plan still launches the old entry, and only that."""
    from robotic_manipulator_rloa_amd.chain_tools import DemonstrationWriter
    case = L.build_case(name, N, K, T_cap)
    rig = LegsRig(case)
    rows, rec, _ = rig.run(poses=False)
    rig.close()
    for keep_contact in (False, True):
        def kept_rows(kept, valid):
            return rows[kept[:, None] & (np.arange(T_cap)[None, :] < valid[:, None])]
        want = gather_demonstrations(rec, np.ones(N, bool), kept_rows, keep_contact)
        w_whole, w_parts = DemonstrationWriter(case.model, D.ORAD), DemonstrationWriter(case.model, D.ORAD, chunk=chunk)
        assert w_whole.legs_actions is None and w_whole.legs_ticks is None
        whole = w_whole.write(case.plan, case.targets, case.obstacles, keep_contact)
        parts = w_parts.write(case.plan, case.targets, case.obstacles, keep_contact)
        assert (w_whole.launches, w_whole.legs_launches) == (0, 1) and w_parts.launches == 0
        assert w_parts.legs_launches == (1 if chunk is None else -(-N * T_cap // chunk)) and w_whole.legs_ticks.numel() >= N * K
        for f, a, b, c in zip(want._fields[:8], whole, parts, want):
            assert a.dtype == b.dtype == c.dtype and a.tobytes() == b.tobytes() == c.tobytes(), f
        assert whole.rows.is_cuda and whole.rows.is_contiguous() and whole.rows_total == parts.rows_total == want.rows_total
        assert np.array_equal(bits(whole.rows.cpu().numpy()), bits(want.rows)) and torch.equal(whole.rows, parts.rows)
    two = D.build_case(name, 3, 130)
    writer = DemonstrationWriter(two.model, D.ORAD)
    writer.write(two.plan, two.targets, two.obstacles)
    assert (writer.launches, writer.legs_launches) == (1, 0) and writer.legs_actions is None
    demos = DemonstrationWriter(case.model, D.ORAD, chunk=chunk).write(case.plan, case.targets, case.obstacles)
    agent = _agent(case.model, action_mode="float")
    stats = agent.add_demonstrations(demos)
    n = demos.rows_total
    assert len(agent.memory) == n == stats["demonstration_rows"] > 0 and stats["demonstrations_kept"] == int(demos.kept.sum())
    back = torch.zeros(n, agent.memory.row_floats, device=DEV)
    agent.memory.gather_rows(torch.arange(n, dtype=torch.int32, device=DEV), back, n)
    torch.cuda.synchronize()
    assert torch.equal(back, demos.rows)
    with pytest.raises(ValueError, match="padding of 0 ticks lies behind"):
        bad = case.plan.n_ticks.copy()
        bad[0, 0] = 0
        writer = DemonstrationWriter(case.model, D.ORAD)
        writer.write(case.plan._replace(n_ticks=bad), case.targets, case.obstacles)
    assert writer.legs_launches == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cut", [("planar3", None), ("iiwa_like7", R.IIWA_CUT)])
def test_joint_path_checker_with_a_shortcut_end_to_end(name, cut):
    """JointPathChecker.check(roadmap=14, shortcut=16) on the two value sets: the round's launches are naf_chain_edge_check's over
    shortcut_nodes of the roadmap polylines; roadmap_search on the device's own shortcut records reproduces nodes, n_nodes and
    length bit for bit under the replacement rule; every query that is not 'roadmap' is bit-equal to the call without shortcut;
    every edge is free at the twin's sure samples; at least one query is shortened."""
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    q0, q1, ob, margin = R.value_queries(name, cut)
    kw = dict(margin=margin, roadmap=R.ROADMAP, **R.VALUE_KW)
    checker = JointPathChecker(R.arm(name)[0], R.ORAD)
    base = checker.check(q0, q1, ob, **kw)
    assert base.roadmap_length is None and base.shortcut_free_edges is None
    before, calls, records_of = checker.edge_launches, [], checker.edge_records

    def recording(nodes, edges, obstacles, S, margin_):
        rec = records_of(nodes, edges, obstacles, S, margin_)
        calls.append((np.array(nodes), np.array(edges), int(S), rec.copy()))
        return rec

    checker.edge_records = recording
    out = checker.check(q0, q1, ob, shortcut=16, **kw)
    rm = base.outcome == "roadmap"
    assert rm.sum() >= 1 and np.array_equal(out.outcome, base.outcome)
    shortcut_calls = calls[before:]                            # (the roadmap round's launches come first, as many as before)
    assert len(calls) > before and checker.edge_launches == before + len(calls)
    for field, x, y in zip(base._fields, out, base):
        assert x.dtype == y.dtype and x[~rm].tobytes() == y[~rm].tobytes(), field
    assert np.array_equal(bits(out.roadmap_length[rm]), bits(base.length[rm])) and np.all(np.isnan(out.roadmap_length[~rm]))
    assert out.nodes.dtype == np.float32 and out.length.dtype == np.float32 and np.all(out.shortcut_free_edges[~rm] == -1)
    done = set()
    for nodes, edges, S, rec in shortcut_calls:
        V = nodes.shape[1]
        assert rec.dtype == np.float32 and np.array_equal(edges, K.roadmap_edges(V)) and nodes.dtype == np.float32
        count, index, length = K.roadmap_search(rec, edges, V)
        for k in range(len(nodes)):
            q = int(np.nonzero(rm & np.all(bits(base.start) == bits(nodes[k, 0]), axis=1) & np.all(bits(base.goal) == bits(nodes[k, 1]), axis=1))[0][0])
            done.add(q)
            assert np.array_equal(bits(nodes[k]), bits(K.shortcut_nodes(base.nodes[q, :base.n_nodes[q]], 16)))
            assert out.shortcut_free_edges[q] == int(np.sum(rec[k, :, 4] == 0))
            replaced = count[k] > 0 and length[k] < base.length[q] and base.length[q] > base.straight_length[q]
            if replaced:
                assert out.n_nodes[q] == count[k] and bits(out.length[q]) == bits(length[k]) and out.samples[q] == S
                assert np.array_equal(bits(out.nodes[q, :count[k]]), bits(nodes[k, index[k, :count[k]]]))
                assert np.all(np.isnan(out.nodes[q, count[k]:]))
            else:
                assert out.n_nodes[q] == base.n_nodes[q] and bits(out.length[q]) == bits(base.length[q])
                assert np.array_equal(bits(out.nodes[q, :out.n_nodes[q]]), bits(base.nodes[q, :base.n_nodes[q]]))
    assert done == set(np.nonzero(rm)[0].tolist())
    shorter = rm & (out.length < base.length)
    print(name, "roadmap", np.nonzero(rm)[0], "x straight", np.round((base.length / base.straight_length)[rm], 2), "->",
          np.round((out.length / out.straight_length)[rm], 2), "nodes", base.n_nodes[rm], "->", out.n_nodes[rm])
    assert shorter.sum() >= 1 and np.all(out.length[rm] <= base.length[rm])
    assert R.edges_free_at_sure_samples(name, out, ob, margin) == int((out.n_nodes[rm] - 1).sum())


def test_framework_shortcut_and_polylines_end_to_end(scratch_cwd, monkeypatch):  # noqa: F811
    """plan_joint_paths(roadmap=14, shortcut=16) -> demonstrate_joint_paths(polylines=True) -> run_training(8, 50, n_envs=16,
    demonstrations=) on test_framework_roadmap_end_to_end's scene: the device's demonstrations carry the twin's outcomes on at
    least 90 % of the queries, 'roadmap' queries contribute rows, the ring holds them and the run's own. Off means off: without the
    new arguments plan_joint_paths(roadmap=14) is bit-equal before and after, a polyline-free demonstrate_joint_paths launches the
    two-leg entry only, and the training stream's digest is what it was."""
    from chain_resume_worker import make_framework
    from robotic_manipulator_rloa_amd import chain_tools
    N = 24
    rng = np.random.default_rng(8)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.15, 0.15, (N, 3))
    targets[-1] = [0.0, 0.0, 2.0]                                      # out of reach
    model, _ = C.arm("iiwa_like7", True)
    stream_agent = _agent(model)
    stream_before = _training_stream_digest(stream_agent, model, False)
    f = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    goal = f.solve_goal_poses(targets, seed=3)
    start = np.tile(f.env.initial_joint_positions, (N, 1))
    obstacles = np.tile(f.env.obstacle_centre if f.env.scene_ranges_on else f.env.obstacle_pos, (N, 1)).astype(np.float64)
    mid = f.env.end_effector(0.5 * (start + np.asarray(goal.joint_positions, np.float64)))
    obstacles[1::2] = np.where(np.asarray(goal.reachable)[1::2, None], mid[1::2], obstacles[1::2])
    kw = dict(obstacles=obstacles, candidates=2, seed=3, resolution=0.05)
    plain = f.plan_joint_paths(targets, roadmap=R.ROADMAP, **kw)
    launches = []
    legs_launch = chain_tools.DemonstrationWriter.launch_legs
    monkeypatch.setattr(chain_tools.DemonstrationWriter, "launch_legs", lambda self, *a: (launches.append(a), legs_launch(self, *a))[1])
    two_leg = f.demonstrate_joint_paths(plain, targets, obstacles=obstacles)
    assert launches == [] and plain.roadmap_length is None and plain.shortcut_free_edges is None
    out = f.plan_joint_paths(targets, roadmap=R.ROADMAP, shortcut=16, **kw)
    rm = out.outcome == "roadmap"
    print({o: int(np.sum(out.outcome == o)) for o in sorted(set(out.outcome))}, "roadmap x straight",
          np.round((out.roadmap_length / out.straight_length)[rm], 2), "->", np.round((out.length / out.straight_length)[rm], 2))
    assert rm.sum() >= 1 and np.array_equal(out.outcome, plain.outcome) and np.all(out.length[rm] <= plain.length[rm])
    for field, x, y in zip(plain._fields, out, plain):
        assert x.dtype == y.dtype and x[~rm].tobytes() == y[~rm].tobytes(), field
    assert out.roadmap_length.shape == out.shortcut_free_edges.shape == (N,) and out.shortcut_free_edges[-1] == -1
    demos = f.demonstrate_joint_paths(out, targets, obstacles=obstacles, frames=400, polylines=True)
    host = f.demonstrate_joint_paths(out, targets, obstacles=obstacles, frames=400, polylines=True, on_device=False)
    assert len(launches) >= 1 and demos.rows.is_cuda and demos.rows_total == demos.rows.shape[0] > f.naf_agent.batch_size
    assert np.array_equal(demos.planned_ticks, host.planned_ticks)
    assert np.array_equal(demos.outcome == "none", (out.candidate < 0) & ~rm) and np.all(two_leg.outcome[rm] == "none")
    same = demos.outcome == host.outcome                      # (a tick inside a band may end one differently: few, if any)
    print("roadmap demonstrations", demos.outcome[rm], demos.frames[rm], "of", demos.planned_ticks[rm], "agree", float(same.mean()))
    assert same.mean() >= 0.9 and np.array_equal(demos.frames[same], host.frames[same])
    via = out.candidate >= 0
    for name in ("outcome", "frames", "planned_ticks", "kept"):      # the one-via queries: the two-leg launch's numbers
        assert np.array_equal(getattr(demos, name)[via], getattr(two_leg, name)[via]), name
    assert int(demos.frames[rm & demos.kept].sum()) >= 1 and demos.rows_total == int(demos.frames[demos.kept].sum())
    f.run_training(8, 50, verbose=False, n_envs=16, demonstrations=demos)
    stats = f.naf_agent.last_run_stats
    assert stats["demonstration_rows"] == demos.rows_total and stats["demonstrations_kept"] == int(demos.kept.sum())
    assert len(f.naf_agent.memory) == demos.rows_total + stats["env_steps"] and stats["updates"] > 0
    # off means off
    n_legs = len(launches)
    again = f.plan_joint_paths(targets, roadmap=R.ROADMAP, **kw)
    for field, x, y in zip(plain._fields, again, plain):
        assert x.tobytes() == y.tobytes(), field
    assert again.nodes.tobytes() == plain.nodes.tobytes() and again.n_nodes.tobytes() == plain.n_nodes.tobytes()
    assert again.roadmap_length is None and len(launches) == n_legs
    assert _training_stream_digest(stream_agent, model, False) == stream_before
