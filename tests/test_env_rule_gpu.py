"""GPU (`-m gpu`): every kernel that states the environment rule held to oracle/env_oracle.py — naf_synth_env_step, naf_chain_env_step
and _step_tagged, naf_chain_env_rollout_step, naf_chain_demo_rows and _rows_legs, naf_replay_gather_rows_hindsight.

The check is the same everywhere (env_rule_common.judge): the float64 distances come from the twin at the pose the kernel itself
reports, env_oracle.rule says what they are worth, and done, the outcome's class and the values +250 / -1000 must be equal, a shaped
reward within the arm's existing tolerance of -(d - 0.05). The distances stay our own kinematics; the rule is the reference's:
tests/test_oracle_golden.py pins env_oracle on fixture G9 on the CPU, and nothing here reads that fixture or the reference.
No tolerance is new: chain_rollout_common.tol_of(model) and its bands (2 tol; 4 tol on the self-clearance) for the chain kernels,
hindsight_common.BAND = 1e-6 and that suite's 1e-5 for the relabelled reward, test_agent_gpu's 3e-6 / 1e-5 for the stand-in.
The cases are env_rule_common's fixed table (E = 100: one full wave and a partial one), which tests/test_env_rule_cpu.py rehearses
on float32 restatements: no constructed case in a band, at most 1 % of the random filler."""
import numpy as np
import pytest
import torch

import chain_rollout_common as C
import env_rule_common as E
from oracle import naf_oracle as O
from test_chain_box_gpu import BoxRig
from test_chain_cell_gpu import CellRig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _clean(census, name):
    print(f"{name}: {census.compared} compared, {census.band} in the band ({census.band_constructed} constructed, "
          f"{census.band_filler} of {census.filler} filler), {census.outcomes}")
    assert census.failures == [], census.failures[:4]
    assert census.band_constructed == 0 and census.band_filler <= 0.01 * max(1, census.filler), census


class StepFace:
    """a BoxRig behind the face env_rule_common.run_step asks for"""

    def __init__(self, rig):
        self.rig, self.off_r, self.off_s2, self.off_d = rig, rig.off_r, rig.off_s2, rig.off_d

    def read(self):
        return self.rig.st.cpu().numpy(), self.rig.obs.cpu().numpy()

    def write_state(self, st):
        self.rig.st.copy_(torch.from_numpy(np.ascontiguousarray(st, np.float32)))

    def step(self, act):
        self.rig.load_actions(act)
        self.rig.launch_step()
        return self.rig.rows.cpu().numpy()


@pytest.mark.parametrize("tagged", [False, True])
@pytest.mark.parametrize("name", E.ARMS)
def test_chain_step_kernels_follow_the_rule(name, tagged):
    """naf_chain_env_step / naf_chain_env_step_tagged on planar3 (bare), iiwa_like7 (pairs, a cell of boxes) and slider4 (prismatic
    joints): one step of the arm's 100 cases; the stored row's reward and done columns, and its next_state's layout."""
    cases = E.build_cases(name)
    model = cases.arm.model
    rig = BoxRig(model, E.E_CASES, tagged=tagged)
    rig.reset(np.array([0.3, 0.2, 0.4]), np.array([3.0, 3.0, 3.0]))
    census, state, pose = E.run_step(cases, StepFace(rig), C.tol_of(model))
    tag = rig.rows.cpu().numpy()[:, -1]
    rig.close()
    _clean(census, f"{name} tagged={tagged}")
    assert state == [] and pose == [], (state[:2], pose[:4])
    assert min(census.outcomes.values()) >= 6 and np.all(tag == (1.0 if tagged else 0.0))


@pytest.mark.parametrize("name", E.ARMS)
def test_chain_rollout_kernel_follows_the_rule(name):
    """naf_chain_env_rollout_step, four launches (the case's action, then none): the outcome code, the score's increment, and the
    hold of an env behind its end."""
    cases = E.build_cases(name)
    model, A = cases.arm.model, cases.arm.model.A
    rig = CellRig(model, E.E_CASES, frames=4)
    rig.reset_given(cases.q0, cases.target, cases.obstacle)
    outs = []
    for t in range(4):
        rig.load_actions(cases.act if t == 0 else np.zeros_like(cases.act))
        rig.launch_rollout()
        outs.append(rig.out.cpu().numpy().copy())
    traj = rig.traj.cpu().numpy()
    rig.close()
    traj[0] = cases.q0
    censuses, not_held = E.judge_rollout(cases, outs, traj, C.tol_of(model))
    for t, census in enumerate(censuses):
        _clean(census, f"{name} launch {t}")
    assert not_held == [] and min(censuses[0].outcomes.values()) >= 6
    ended = outs[0][:, 0] != 0
    assert 12 <= ended.sum() < E.E_CASES and np.all(outs[3][~ended, 1] == 4.0)


@pytest.mark.parametrize("legs", [2, 3])
def test_demonstration_kernels_follow_the_rule(legs):
    """naf_chain_demo_rows (two legs) and naf_chain_demo_rows_legs (three), iiwa_like7 among its boxes, N = 8, T = 16: the reward and
    done of every row of every demonstration, the row that arrives on the constructed pose among them."""
    from test_chain_demo_gpu import DemoRig
    from test_chain_legs_gpu import LegsRig
    case = E.build_demo_case(legs)
    rig = (DemoRig if legs == 2 else LegsRig)(case)
    rows, records, _ = rig.run()
    rig.close()
    census, judged, all_built = E.judge_demo_rows(case, rows, C.tol_of(case.model))
    _clean(census, f"legs {legs}: {judged} rows")
    assert all_built and judged == int(records[:, 0].sum())
    want = {"target_in": 1, "obstacle_in": 2, "self_in": 3, "cell_in": 4, "reached_self": 1, "obstacle_self": 2}
    for n, kind in enumerate(case.kind):
        if kind in want:
            assert (records[n, 0], records[n, 1]) == (case.tick + 1, want[kind]), (kind, records[n])
        else:
            assert records[n, 0] > case.tick + 1, (kind, records[n])


def test_hindsight_gather_follows_the_rule():
    """naf_replay_gather_rows_hindsight on the synthetic ring (23, 7, E = 3), horizon 8, ratio 1, whole ring rows, 16 of them put
    16e-6 either side of the threshold: every relabelled row's reward and done are env_oracle.relabelled of the distance between
    its own end-effector and goal columns; contact rows, and every row not relabelled, are the plain gather's byte for byte."""
    from test_hindsight_gpu import RingRig
    from robotic_manipulator_rloa_amd.utils import hindsight as H
    ring, idx_np, u, k0, built = E.hindsight_cases()
    S, A, n_env = E.HINDSIGHT_SHAPE
    rig = RingRig(ring)
    idx = torch.from_numpy(idx_np.copy()).to(DEV)
    ld = H.row_floats(S, A)
    plain = rig.plain(idx, ld)
    got, k = rig.hindsight(idx, ld, E.HINDSIGHT_HORIZON, E.HINDSIGHT_RATIO)
    assert rig.bad() == 0
    rig.close()
    failures, census = E.judge_hindsight(plain, got, k, built)
    print("hindsight:", census)
    assert failures == [], failures[:4]
    assert census["band_built"] == 0 and census["band"] <= 0.01 * census["compared"] and census["compared"] >= 100
    off_r, off_d = O.row_offsets(S, A)[1], O.row_offsets(S, A)[3]
    took = (k >= 0) & (built != 0)
    assert took.sum() >= 2 * E.HINDSIGHT_PER_SIDE
    assert np.all(got[took & (built < 0), off_r] == 250.0) and np.all(got[took & (built > 0), off_d] == 0.0)
    assert np.sum(plain[:, off_r] == -1000.0) >= 8            # contact rows were among the gathered ones


@pytest.mark.parametrize("A", [6, 8])
def test_synthetic_env_kernel_follows_the_rule(A):
    """naf_synth_env_step — the launch of the vector step's separate form (engine.DeviceEnvLoop with fused=False) — on 100 cases of the
    A-joint stand-in: reward, done and the row's next_state columns."""
    from robotic_manipulator_rloa_amd import _lib
    lib = _lib.load()
    cases = E.build_synth_cases(A)
    n, S = E.E_CASES, 2 * A + 9
    _, off_r, off_s2, off_d = O.row_offsets(S, A)
    st = torch.zeros(n, lib.naf_synth_env_state_floats(A), device=DEV)
    obs = torch.zeros(n, S, device=DEV)
    rows = torch.zeros(n, lib.naf_replay_row_floats(S, A), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.naf_synth_env_reset(st.data_ptr(), obs.data_ptr(), n, A, 5, 0, None, 0, stream) == 0
    host = st.cpu().numpy()
    host[:, :A], host[:, 8:11], host[:, 11:14] = cases.q0, cases.target, cases.obstacle
    st.copy_(torch.from_numpy(host))
    act = torch.from_numpy(np.ascontiguousarray(cases.act, np.float32)).to(DEV)
    assert lib.naf_synth_env_step(st.data_ptr(), act.data_ptr(), rows.data_ptr(), obs.data_ptr(), n, A, 5, None, 0, None, 0, stream) == 0
    row = rows.cpu().numpy()
    s2 = row[:, off_s2:off_s2 + S]
    q, qd = s2[:, :A].astype(np.float64), s2[:, A:2 * A].astype(np.float64)
    want_q = cases.q0 + cases.act / 240.0
    assert np.all(np.abs(q - want_q) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want_q)))
    dist = E.synth_distances(A, q, cases.target, cases.obstacle)
    census = E.judge(cases.arm, dist, row[:, off_r], row[:, off_d], E.REWARD_TOL_SYNTH, cases.constructed, band_tol=E.TOL_SYNTH)
    _clean(census, f"synthetic A={A}")
    assert min(census.outcomes.values()) >= 10
    assert E.judge_state(cases.arm, q, qd, dist, cases.target, cases.obstacle, s2, E.TOL_SYNTH) == []
