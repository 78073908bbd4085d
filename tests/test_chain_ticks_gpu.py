"""GPU (`-m gpu`): naf_chain_demo_rows_ticks (csrc/chain_env.hip) through the C ABI with poisoned pad rows behind every output and
poisoned action entries at k >= T_n — fed the actions of the two-leg and the K-leg cases against those entries bit for bit, on the
tick cases against the step kernel it restates and the float64 rule (environment/tick_demo.py, demonstration_rows_host); placement
independence and the refusals; chain_tools.DemonstrationWriter with a TickPlan; and plan_joint_paths -> plan_trajectories ->
demonstrate_trajectories -> run_training end to end. tests/test_chain_ticks_cpu.py rehearses every case with a float32 restatement."""
import numpy as np
import pytest
import torch

import chain_demo_common as D
import chain_legs_common as L
import chain_roadmap_common as R
import chain_rollout_common as C
import chain_ticks_common as X
from test_chain_demo_gpu import CASES as TWO_LEG_CASES
from test_chain_demo_gpu import PAD, DemoRig, scratch_cwd  # noqa: F401
from test_chain_env_gpu import _agent
from test_chain_legs_gpu import LegsRig, same_bits
from test_chain_rollout_gpu import IIWA_RANGED, _training_stream_digest
from test_chain_ticks_cpu import ARGUMENT_ERRORS

from robotic_manipulator_rloa_amd.environment import tick_demo as K
from robotic_manipulator_rloa_amd.environment.kinematic import gather_demonstrations, reach_table
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
bits = D.bits


class TicksRig(DemoRig):
    """test_chain_demo_gpu.DemoRig with the launch of naf_chain_demo_rows_ticks: a table [N][T_cap][A] whose entries at k >= T_n are
    NaN, and the planned ticks [N]; steps(), the composed form, is DemoRig's as it stands (it reads demo_actions of case.plan)."""

    def __init__(self, case, table, counts):
        super().__init__(case)
        self.actions = torch.from_numpy(np.ascontiguousarray(table, np.float32)).to(DEV)
        self.ticks = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(DEV)
        assert self.actions.shape == (self.N, self.T, self.A) and self.ticks.shape == (self.N,)

    def call(self, poses=True, stream=None, **over):
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        p = lambda t: t.data_ptr()      # noqa: E731
        a = dict(h=self.h, q=p(self.q_start), a=p(self.actions), n=p(self.ticks), t=p(self.targets), o=p(self.obstacles), rad=D.ORAD,
                 N=self.N, T=self.T, rows=p(self.rows), rf=self.rf, rec=p(self.records))
        a.update(over)
        rf = self.rf + 1 if a["rf"] is None else a["rf"]
        return self.lib.naf_chain_demo_rows_ticks(a["h"], a["q"], a["a"], a["n"], a["t"], a["o"], a["rad"], a["N"], a["T"], a["rows"], rf,
                                                  a["rec"], p(self.poses) if poses else None, st)

    run = LegsRig.run


def tick_rig(case):
    return TicksRig(case, X.poisoned_table(case), np.asarray(case.tick_plan.planned_ticks, np.int32))


# ---- 5. against the two entries it generalises -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [("demo",) + tuple(c) for c in TWO_LEG_CASES] + [("legs",) + tuple(c) for c in L.CASES])
def test_ticks_are_the_legs_kernels_bit_for_bit(case_id):
    """For every case of test_chain_demo_gpu and of chain_legs_common, the tick entry fed demo_actions(plan, T_cap) as float32 —
    NaN behind each demonstration's own ticks — and the sum of its counts gives rows, records and poses bit for bit those of
    naf_chain_demo_rows / naf_chain_demo_rows_legs, poison where nothing is written included, with and without poses_out."""
    if case_id[0] == "demo":
        case = D.build_case(*case_id[1:])
        old = DemoRig(case)
    else:
        case = L.build_case(*case_id[1:])
        old = LegsRig(case)
    want = old.run()
    old.close()
    rig = TicksRig(case, *X.table_of(case.plan, case.T_cap))
    got, plain = rig.run(), rig.run(poses=False)
    rig.close()
    assert same_bits(got, want) and same_bits(plain[:2], want[:2])


# ---- 6. the tick cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,T_cap", X.CASES)
def test_tick_rows_against_the_step_kernel_and_the_rule(name, N, T_cap):
    """One tick case through the C ABI, poses_out on, under the split test_legs_rows_against_the_step_kernel_and_the_rule applies.
    Against the composed form (reset_given, then T_cap x naf_chain_env_step fed the same table): for the rows up to each
    demonstration's first done, joint positions, velocities, actions, target, obstacle and the zeros bit for bit; the end effector
    within 1 tol; reward class and done equal outside the bands (at most 1 % of the ticks inside); the record's count the composed
    form's first done; counts and codes the twin's where no band tick precedes. Against the float64 rule and for chain exactness:
    chain_demo_common.check_rows. In addition the device's poses are within the derived tracking bound of the float64 law (clipped
    into the limits, which the arm cannot leave) at the ticks — they are, bit for bit, the poses the host predicted when it formed
    the actions."""
    case = X.build_case(name, N, T_cap)
    rig = tick_rig(case)
    rows, rec, poses = rig.run()
    plain_rows, plain_rec, _ = rig.run(poses=False)
    ref = rig.steps()
    rig.close()
    assert np.array_equal(bits(np.nan_to_num(rows)), bits(np.nan_to_num(plain_rows))) and np.array_equal(bits(rec), bits(plain_rec))
    D.check_rows(case, rows, rec, poses)
    tp = case.tick_plan
    upto = np.arange(T_cap + 1)[None, :] <= tp.rows[:, None]
    err = np.where(upto, np.abs(np.nan_to_num(poses).astype(np.float64) - X.clipped_law(case)).max(axis=2), 0.0).max(axis=1)
    bound = X.device_tracking_bound(case)
    print(f"{name} N={N} T_cap={T_cap}: tracking error on the device {err.max():.3g} (bound {bound.max():.3g})")
    assert np.all(err <= bound)
    _, want_poses, _ = K.tick_recurrence(tp.q_start, case.law, case.twin.joint_limits(), True)
    assert np.array_equal(bits(np.where(upto[..., None], np.nan_to_num(poses), 0)), bits(np.where(upto[..., None], want_poses, 0)))
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
    err_ee = float(np.abs(got[:, ee].astype(np.float64) - want[:, ee]).max())
    assert err_ee <= tol
    sure = ~band
    assert np.array_equal(got[sure, off_d], want[sure, off_d])
    r_got, r_want = got[sure, S + A].astype(np.float64), want[sure, S + A].astype(np.float64)
    terminal = (r_want == 250.0) | (r_want == -1000.0)
    assert np.array_equal(r_got[terminal], r_want[terminal]) and np.abs(r_got - r_want)[~terminal].max(initial=0.0) <= tol
    first_band = np.array([in_band[n, :valid[n]].any() for n in range(N)])
    ref_done = ref[..., off_d] == 1.0
    ref_valid = np.where(ref_done.any(axis=1), ref_done.argmax(axis=1) + 1, T_cap + 1)
    assert np.array_equal(valid[~first_band], np.minimum(ref_valid, tp.rows)[~first_band])
    _, h_rec, _, _ = case.host()
    if not first_band.any():
        assert np.array_equal(rec[:, 0], h_rec[:, 0]) and np.array_equal(rec[:, 1], h_rec[:, 1])
    assert np.array_equal(rec[:, 6], tp.planned_ticks)
    if T_cap >= X.ROLE_TICKS and not first_band.any():      # every role ends on the device as it was built to
        assert np.all(X.ends_as_built(case.role, rec[:, 1])) and np.all((rec[:, 0] < rec[:, 6])[case.role == 0])
    if T_cap >= X.LIMIT_TICKS and any(j.limited for j in case.model.joints):
        # the limit role: ON the limit at ticks lanes - 1 and lanes — across the first pass boundary — with velocity slot 0 there
        lanes = D.lanes_of(case.model)
        lo, hi = [v.astype(np.float32) for v in case.twin.joint_limits()]
        src = [s_ for s_, _ in case.model.slots]
        for n in np.flatnonzero(case.role == 4):
            for t in (lanes - 1, lanes):
                on = [m for m in range(A) if (poses[n, t + 1, m] == hi[m] and tp.actions[n, t, m] > 0) or (poses[n, t + 1, m] == lo[m] and tp.actions[n, t, m] < 0)]
                assert on and valid[n] > t, (n, t)
                for m in on:
                    assert rows[n, t, off_s2 + A + src.index(m)] == 0.0


@pytest.mark.parametrize("name", X.BOUNDARY_NAMES)
def test_a_first_done_on_the_pass_boundary(name):
    """chain_ticks_common.boundary_case through the C ABI: demonstrations whose first done is walked by the last lane of pass 0
    (lanes - 1 valid rows) and by lane 0 of pass 1 (lanes valid rows; its row's action comes from the carry), by reaching and by
    touching. Counts and codes are the twin's, the rows up to the first done are the composed form's in every float the split
    calls exact — the action of row lanes - 1 among them — and chain_demo_common.check_rows holds."""
    case = X.boundary_case(name)
    lanes = D.lanes_of(case.model)
    rig = tick_rig(case)
    rows, rec, poses = rig.run()
    ref = rig.steps()
    rig.close()
    D.check_rows(case, rows, rec, poses)
    assert rec[:, 0].tolist() == [lanes - 1, lanes, lanes - 1, lanes] and rec[:, 1].tolist() == [1, 1, 2, 2]
    A, S, off_s2, off_d = rig.A, rig.S, rig.off_s2, rig.off_d
    live = np.arange(case.T_cap)[None, :] < rec[:, :1].astype(np.int64)
    exact = np.zeros(rig.rf, bool)
    for lead in (0, off_s2):
        exact[lead:lead + 2 * A] = exact[lead + 2 * A + 3:lead + 2 * A + 9] = True
    exact[S:S + A] = exact[S + A + 1:off_s2] = exact[off_d + 1:] = True
    assert np.array_equal(bits(rows[live][:, exact]), bits(ref[live][:, exact]))
    assert np.array_equal(rows[live][:, off_d], ref[live][:, off_d]) and np.all(rows[np.arange(4), rec[:, 0].astype(int) - 1, off_d] == 1.0)
    assert np.array_equal(bits(rows[:, lanes - 1, S:S + A][rec[:, 0] == lanes]), bits(case.tick_plan.actions[:, lanes - 1][rec[:, 0] == lanes]))


# ---- 7. placement and refusals -----------------------------------------------------------------------------------------------------
def test_placement_independence_through_the_c_abi():
    """A demonstration of the 16 x 256 case gives the same rows, record and poses alone at index 0 of a launch of one as inside
    the launch of 16, bit for bit; a launch on a side stream gives the current stream's bits."""
    case = X.build_case("iiwa_like7", 16, 256)
    rig = tick_rig(case)
    big = rig.run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = rig.run(stream=side.cuda_stream)
    rig.close()
    assert same_bits(big, on_side)
    for n in (9, 2):
        one = tick_rig(case.sub(n))
        alone = one.run()
        one.close()
        for a, b in zip(big, alone):
            assert np.array_equal(bits(np.nan_to_num(a[n])), bits(np.nan_to_num(b[0])))


def test_argument_errors_launch_nothing():
    """Every refusal include/naf_hip.h names returns NAF_ERR_ARG with a real handle and real buffers, and the poisoned outputs are
    still poisoned behind them all: nothing was launched."""
    case = X.build_case("planar3", 5, 130)
    rig = tick_rig(case)
    for t in (rig.rows, rig.records, rig.poses):
        t.fill_(float("nan"))
    for kw in ARGUMENT_ERRORS:
        assert rig.call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.isnan(rig.rows).all() and torch.isnan(rig.records).all() and torch.isnan(rig.poses).all()
    _, rec, _ = rig.run()
    assert not np.isnan(rec).any()
    rig.close()


# ---- 8. the writer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,T_cap,chunk", [("iiwa_like7", 16, 256, 2 * 256), ("long12", 5, 130, 130), ("slider4", 16, 256, None)])
def test_demonstration_writer_with_a_tick_plan_across_chunks_and_the_ring(name, N, T_cap, chunk):
    """chain_tools.DemonstrationWriter with a TickPlan in forced small chunks and in one chunk gives the kept rows of one C-ABI
    launch, in query order then tick order, and its numbers, through naf_chain_demo_rows_ticks alone; after add_demonstrations on a
    fresh agent the ring reads back exactly those rows. A two-leg plan still launches only the two-leg entry and a K-leg plan only
    the legs entry, and neither allocates the tick staging."""
    from robotic_manipulator_rloa_amd.chain_tools import DemonstrationWriter
    case = X.build_case(name, N, T_cap)
    rig = tick_rig(case)
    rows, rec, _ = rig.run(poses=False)
    rig.close()
    tp = case.tick_plan
    for keep_contact in (False, True):
        def kept_rows(kept, valid):
            return rows[kept[:, None] & (np.arange(T_cap)[None, :] < valid[:, None])]
        want = gather_demonstrations(rec, np.ones(N, bool), kept_rows, keep_contact)
        w_whole, w_parts = DemonstrationWriter(case.model, D.ORAD), DemonstrationWriter(case.model, D.ORAD, chunk=chunk)
        assert w_whole.tick_actions is None and w_whole.tick_counts is None
        whole = w_whole.write(tp, case.targets, case.obstacles, keep_contact)
        parts = w_parts.write(tp, case.targets, case.obstacles, keep_contact)
        assert (w_whole.launches, w_whole.legs_launches, w_whole.ticks_launches) == (0, 0, 1) and w_whole.legs_actions is None
        assert (w_parts.launches, w_parts.legs_launches) == (0, 0) and w_parts.ticks_launches >= (1 if chunk is None else 2)
        for f, a, b, c in zip(want._fields[:8], whole, parts, want):
            assert a.dtype == b.dtype == c.dtype and a.tobytes() == b.tobytes() == c.tobytes(), f
        assert whole.rows.is_cuda and whole.rows.is_contiguous() and whole.rows_total == parts.rows_total == want.rows_total
        assert np.array_equal(bits(whole.rows.cpu().numpy()), bits(want.rows)) and torch.equal(whole.rows, parts.rows)
    two = D.build_case(name, 3, 130)
    writer = DemonstrationWriter(two.model, D.ORAD)
    writer.write(two.plan, two.targets, two.obstacles)
    assert (writer.launches, writer.legs_launches, writer.ticks_launches) == (1, 0, 0) and writer.tick_actions is None
    legs = L.build_case(name, 3, 3, 130)
    writer.write(legs.plan, legs.targets, legs.obstacles)
    assert (writer.launches, writer.legs_launches, writer.ticks_launches) == (1, 1, 0) and writer.tick_actions is None
    demos = DemonstrationWriter(case.model, D.ORAD, chunk=chunk).write(tp, case.targets, case.obstacles)
    agent = _agent(case.model, action_mode="float")
    stats = agent.add_demonstrations(demos)
    n = demos.rows_total
    assert len(agent.memory) == n == stats["demonstration_rows"] > 0 and stats["demonstrations_kept"] == int(demos.kept.sum())
    back = torch.zeros(n, agent.memory.row_floats, device=DEV)
    agent.memory.gather_rows(torch.arange(n, dtype=torch.int32, device=DEV), back, n)
    torch.cuda.synchronize()
    assert torch.equal(back, demos.rows)


# ---- 9. end to end -----------------------------------------------------------------------------------------------------------------
def test_framework_trajectories_as_demonstrations_end_to_end(scratch_cwd, monkeypatch):  # noqa: F811
    """plan_joint_paths(roadmap, shortcut) -> plan_trajectories(certify=True, clearance_margin above the tracking bound times the
    arm's reach) -> demonstrate_trajectories -> run_training(8, 50, n_envs=16, demonstrations=) on
    test_framework_shortcut_and_polylines_end_to_end's scene (N = 24): the device's outcomes are the twin's on at least 90 % of the
    queries; NO 'certified' trajectory's demonstration ends in contact; the ring holds the rows. Off means off: the training
    stream's digest is unchanged, and demonstrate_joint_paths launches what it launched — no tick launch, no tick staging."""
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
    paths = f.plan_joint_paths(targets, obstacles=obstacles, candidates=2, seed=3, resolution=0.05, roadmap=R.ROADMAP, shortcut=16)
    launches = []
    tick_launch = chain_tools.DemonstrationWriter.launch_ticks
    monkeypatch.setattr(chain_tools.DemonstrationWriter, "launch_ticks", lambda self, *a: (launches.append(a), tick_launch(self, *a))[1])
    old = f.demonstrate_joint_paths(paths, targets, obstacles=obstacles, polylines=True)
    writer = f.arm_planner.tools["demonstrations"][1]
    counters = (writer.launches, writer.legs_launches)
    assert launches == [] and writer.tick_actions is None and old.tracking_error is None
    # a pose within e of the law in every joint moves no capsule point by more than e x the column sums of the reach table
    gain = float(reach_table(f.env.model).sum(axis=0).max())
    e = float(K.tracking_radius(np.pi)) * 2.0                           # r (1 + a run of one): no run is longer at max_velocity 0.5
    margin = 0.002
    assert margin > e * gain
    traj = f.plan_trajectories(paths, obstacles=obstacles, max_velocity=0.5, max_acceleration=4.0, certify=True, clearance_margin=margin)
    demos = f.demonstrate_trajectories(traj, targets, obstacles=obstacles, frames=400)
    host = f.demonstrate_trajectories(traj, targets, obstacles=obstacles, frames=400, on_device=False)
    assert len(launches) >= 1 and demos.rows.is_cuda and demos.rows_total == demos.rows.shape[0] > f.naf_agent.batch_size
    assert np.array_equal(demos.planned_ticks, host.planned_ticks) and np.array_equal(demos.outcome == "none", traj.outcome == "none")
    assert np.array_equal(demos.tracking_error, host.tracking_error, equal_nan=True) and np.nanmax(demos.tracking_error) <= e
    assert not demos.saturated_ticks.any()
    same = demos.outcome == host.outcome                      # (a tick inside a band may end one differently: few, if any)
    cert = traj.outcome == "certified"
    print({o: int(np.sum(traj.outcome == o)) for o in sorted(set(traj.outcome))}, {o: int(np.sum(demos.outcome == o)) for o in sorted(set(demos.outcome))},
          "agree", float(same.mean()), "certified", int(cert.sum()), "tracking", float(np.nanmax(demos.tracking_error)))
    assert same.mean() >= 0.9 and np.array_equal(demos.frames[same], host.frames[same])
    assert cert.sum() >= 1 and not np.isin(demos.outcome[cert], ("obstacle", "self", "workcell")).any()
    assert demos.rows_total == int(demos.frames[demos.kept].sum())
    f.run_training(8, 50, verbose=False, n_envs=16, demonstrations=demos)
    stats = f.naf_agent.last_run_stats
    assert stats["demonstration_rows"] == demos.rows_total and stats["demonstrations_kept"] == int(demos.kept.sum())
    assert len(f.naf_agent.memory) == demos.rows_total + stats["env_steps"] and stats["updates"] > 0
    # off means off
    n_ticks = len(launches)
    again = f.demonstrate_joint_paths(paths, targets, obstacles=obstacles, polylines=True)
    assert len(launches) == n_ticks and (writer.launches - counters[0], writer.legs_launches - counters[1]) == counters
    for name in ("outcome", "frames", "planned_ticks", "kept"):
        assert np.array_equal(getattr(again, name), getattr(old, name)), name
    assert torch.equal(again.rows, old.rows)
    assert _training_stream_digest(stream_agent, model, False) == stream_before
