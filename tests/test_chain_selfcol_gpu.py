"""GPU (`-m gpu`): the self-collision instantiation of csrc/chain_env.hip against the float64 twin (environment/kinematic.py) —
clearances through naf_chain_env_probe, reward class and done through naf_chain_env_step — beside the obstacle rule, against
the instantiation without it, under graph capture, and through the framework end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import naf_oracle as O
from test_chain_env_cpu import ARMS, model_of, path
from test_chain_env_gpu import DEV, ORAD, Rig, _loop_run
from test_chain_selfcol_cpu import THETA, scattered_q, selfcol_model, spiky_model

from robotic_manipulator_rloa_amd.environment.kinematic import KinematicEnvironment
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT

pytestmark = pytest.mark.gpu
FREE_START = ("planar3", "iiwa_like7", "arm_with_gripper", "standin8")      # the others' start pose is in self-contact
ROLLOUT_FRAMES = 4


def probe(rig):
    out = torch.zeros(rig.E, 5, device=DEV)
    assert rig.lib.naf_chain_env_probe(rig.h, rig.st.data_ptr(), out.data_ptr(), rig.E, rig.stream) == 0
    return out.cpu().numpy()


def put(rig, q=None, target=None, obstacle=None):
    st, A = rig.st.cpu().numpy(), rig.A
    for lo, v in ((0, q), (A, target), (A + 3, obstacle)):
        if v is not None:
            st[:, lo:lo + np.shape(v)[-1]] = v
    rig.st.copy_(torch.from_numpy(st))


class Tally:
    def __init__(self):
        self.steps = self.skipped = self.self_only = self.nothing = 0
        self.worst = 0.0


def check(rig, twin, q, target, obstacle, tol, tally, got_probe, row):
    """One vector step (its row) and the probe taken before it against the twin at the joint values q the step ended at."""
    E = rig.E
    ee = twin.end_effector(q)
    dist = np.linalg.norm(ee - target, axis=-1)
    clear = twin.clearance(q, obstacle)
    self_clear = twin.self_clearance(q)
    if got_probe is not None:
        assert np.abs(got_probe[:, :3] - ee).max() <= tol
        assert np.abs(got_probe[:, 3] - (clear - ORAD)).max() <= 2 * tol
        err = np.abs(got_probe[:, 4] - self_clear).max()
        tally.worst = max(tally.worst, float(err))
        assert err <= 4 * tol, (err, 4 * tol)
    assert np.all(dist > 0.05 + 2 * tol) and np.all(clear > ORAD + 2 * tol)       # the scene is far away: only self-contact ends a step
    reward, done = row[:, rig.off_r], row[:, rig.off_d]
    hit = self_clear < 0.0
    near = np.abs(self_clear) <= 4 * tol
    tally.steps += E
    tally.skipped += int(near.sum())
    tally.self_only += int((hit & ~near).sum())
    tally.nothing += int((~hit & ~near).sum())
    ok = near | np.where(hit, (reward == -1000.0) & (done == 1.0), (reward > -1000.0) & (reward < 0.0) & (done == 0.0))
    assert np.all(ok), (np.nonzero(~ok)[0][:5], self_clear[~ok][:5], reward[~ok][:5], done[~ok][:5])


def free_poses(model, twin, n, rng):
    """n poses out of self-contact, found with the twin alone: from the straight arm, 30 rounds that keep the best of 256 normal
    perturbations (sigma 0.15 rad) by self-clearance, then poses within +-0.05 rad of where that ends which the twin finds free."""
    lo = np.array([j.lower if j.limited else -np.pi for j in model.joints])
    hi = np.array([j.upper if j.limited else np.pi for j in model.joints])
    q0 = np.zeros(model.A)
    best = twin.self_clearance(q0)
    for _ in range(30):
        cand = np.clip(q0 + 0.15 * rng.normal(size=(256, model.A)), lo, hi)
        c = twin.self_clearance(cand)
        if c.max() > best:
            q0, best = cand[np.argmax(c)], c.max()
    assert best > 0.0, best
    out = []
    while sum(len(o) for o in out) < n:
        q = np.clip(q0 + rng.uniform(-0.05, 0.05, (1024, model.A)), lo, hi).astype(np.float32)
        out.append(q[twin.self_clearance(q.astype(np.float64)) >= 0.0])
    return np.concatenate(out)[:n]


@pytest.mark.parametrize("E", [1, 64, 100])
@pytest.mark.parametrize("name", ["planar3", "arm_with_gripper", "standin8", "long12", "long32", "iiwa_like7"])
def test_selfcol_kernel_against_twin(name, E):
    """Teacher-forced, target and obstacle out of reach (3 reach above / below the base), the option on:
    (a) scattered configurations (uniform inside the limits, action 0): 2000 vector steps at E = 1, 300 otherwise;
    (b) arms whose start pose is free: 300 steps of N(0, 1) actions from reset in episodes of up to 4 steps; the others (long12,
        long32: 93 % and 99.8 % of their scattered poses are in self-contact, too few free ones to count): ceil(192 / E) vector
        steps over free poses around one that free_poses() finds with the twin alone.
    Through probe: end effector within tol = 16 A 2^-24 reach, obstacle clearance within 2 tol, self-clearance within 4 tol (2 tol
    for a pair's end points, 2 tol for the float32 pair formula, which test_float32_rehearsal_of_the_pair_formula holds to it).
    Through step: reward class and done equal to the twin's, except steps whose twin self-clearance is within 4 tol of 0, which are
    skipped: at most 1 % of the case's steps. A case counts, outside that band, >= 100 steps that end by self-contact alone and
    >= 100 by nothing, or fails as vacuous; iiwa_like7, where no self-contact is reachable, is the no-false-alarm case and is
    exempt from the first count."""
    n = 2000 if E == 1 else 300
    model, batches = scattered_q(name, E, n)
    A = model.A
    twin = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), ORAD)
    tol = 16 * A * 2.0 ** -24 * model.reach
    target = np.float32([0.0, 0.0, 3.0 * model.reach]).astype(np.float64)
    obstacle = np.float32([0.0, 0.0, -3.0 * model.reach]).astype(np.float64)
    tg, ob = np.broadcast_to(target, (E, 3)), np.broadcast_to(obstacle, (E, 3))
    rig = Rig(model, E, target, obstacle)
    tally = Tally()
    rng = np.random.default_rng(12)
    zero = np.zeros((E, A), np.float32)
    if name in FREE_START:
        lo = np.array([j.lower if j.limited else -np.inf for j in model.joints])
        hi = np.array([j.upper if j.limited else np.inf for j in model.joints])
        for _ in range(300):
            q_prev = rig.st[:, :A].cpu().numpy().astype(np.float64)
            act = rng.normal(size=(E, A)).astype(np.float32)
            row = rig.step(act, max_frames=ROLLOUT_FRAMES)
            check(rig, twin, np.clip(q_prev + DT * act.astype(np.float64), lo, hi), tg, ob, tol, tally, None, row)
    else:
        batches = batches + list(free_poses(model, twin, -(-192 // E) * E, rng).reshape(-1, E, A))
    for q in batches:
        put(rig, q=q)
        got = probe(rig)
        check(rig, twin, q.astype(np.float64), tg, ob, tol, tally, got, rig.step(zero))
    rig.close()
    print(f"{name} E={E}: steps {tally.steps} skipped {tally.skipped} self-contact only {tally.self_only} nothing {tally.nothing} "
          f"worst self-clearance error {tally.worst:.3e} (4 tol = {4 * tol:.3e})")
    assert tally.steps >= n * E
    assert tally.skipped <= 0.01 * tally.steps, (tally.skipped, tally.steps)
    assert tally.nothing >= 100, tally.nothing
    if name != "iiwa_like7":
        assert tally.self_only >= 100, tally.self_only
    else:
        assert tally.self_only == 0


def test_obstacle_and_self_contact_together():
    """planar3 folded as in test_planar3_folded_onto_itself, one env per scene: self-contact alone, obstacle contact alone, both,
    neither, and the target reached while in self-contact (+250: the target is tested first)."""
    model = selfcol_model("planar3")
    twin = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), ORAD)
    q2 = 1.5 * np.pi - THETA
    folded, open_ = [0.0, THETA + 0.2, q2], [0.0, THETA - 0.2, q2]
    q = np.float32([folded, open_, folded, open_, folded])
    ee = twin.end_effector(q.astype(np.float64))
    far = np.full((5, 3), 3.0)
    target, obstacle = far.copy(), -far
    obstacle[1], obstacle[2] = ee[1], ee[2]
    target[4] = ee[4]
    rig = Rig(model, 5, far[0], -far[0])
    put(rig, q=q, target=target.astype(np.float32), obstacle=obstacle.astype(np.float32))
    before = rig.st.cpu().numpy().copy()
    p = probe(rig)
    np.testing.assert_array_equal(rig.st.cpu().numpy(), before)               # probe changes no state
    assert [bool(v < 0) for v in p[:, 4]] == [True, False, True, False, True]
    assert [bool(v < 0) for v in p[:, 3]] == [False, True, True, False, False]
    assert np.abs(p[:, 4] - twin.self_clearance(q.astype(np.float64))).max() <= 4 * 16 * 3 * 2.0 ** -24 * model.reach
    row = rig.step(np.zeros((5, 3), np.float32))
    assert list(row[:3, rig.off_r]) == [-1000.0, -1000.0, -1000.0] and -10.0 < row[3, rig.off_r] < 0.0
    assert row[4, rig.off_r] == 250.0
    assert list(row[:, rig.off_d]) == [1.0, 1.0, 1.0, 0.0, 1.0]
    rig.close()
    # without pairs the probe reports +inf and the folded arm goes on
    off = Rig(model_of("planar3"), 5, far[0], -far[0])
    put(off, q=q, target=far.astype(np.float32), obstacle=(-far).astype(np.float32))
    assert np.all(np.isposinf(probe(off)[:, 4]))
    assert np.all(off.step(np.zeros((5, 3), np.float32))[:, off.off_d] == 0.0)
    off.close()


def test_the_two_instantiations_walk_alike():
    """iiwa_like7 has no reachable self-contact after pruning, so the option changes nothing it computes: 300 steps from reset,
    same seed and actions, rows, observations and env_state bit for bit those of the kernel without the pair phase."""
    on = Rig(selfcol_model("iiwa_like7"), 100, (0.45, 0.3, 0.6), (0.35, 0.2, 0.45), jitter=0.02, record_slots=8)
    off = Rig(model_of("iiwa_like7"), 100, (0.45, 0.3, 0.6), (0.35, 0.2, 0.45), jitter=0.02, record_slots=8)
    assert len(on.m.self_pairs) == 18 and not off.m.self_pairs
    rng = np.random.default_rng(3)
    for _ in range(300):
        act = (3.0 * rng.normal(size=(100, 7))).astype(np.float32)
        before = on.st.cpu().numpy().copy()
        assert np.all(probe(on)[:, 4] > 0.0)
        np.testing.assert_array_equal(on.st.cpu().numpy(), before)
        a, b = on.step(act, max_frames=25), off.step(act, max_frames=25)
        assert a.tobytes() == b.tobytes()
        assert on.obs.cpu().numpy().tobytes() == off.obs.cpu().numpy().tobytes()
        assert on.st.cpu().numpy().tobytes() == off.st.cpu().numpy().tobytes()
        assert on.recs.cpu().numpy().tobytes() == off.recs.cpu().numpy().tobytes()
    assert np.all(on.st[:, 7 + 8].cpu().numpy() >= 300 // 25)                 # (auto-resets took part)
    on.close()
    off.close()


def near_contact_planar3(**over):
    """planar3 starting 0.05 rad before the fold of test_planar3_folded_onto_itself, +-0.1 on every joint: the start pose is free,
    about a third of the reset poses are not, and a few steps carry others across."""
    ee, involved, fixed, _, _ = ARMS["planar3"]
    kw = dict(manipulator_file=path("planar3"), endeffector_index=ee, fixed_joints=fixed, involved_joints=involved,
              target_position=[0.3, 0.3, 0.5], obstacle_position=[2.0, 2.0, 2.0],
              initial_joint_positions=[0.0, THETA - 0.05, 1.5 * np.pi - THETA], initial_positions_variation_range=[0.1, 0.1, 0.1],
              link_radius=0.03, consider_autocollision=True)
    kw.update(over)
    return kw


def test_selfcol_determinism_and_graph_equals_direct_launches():
    """The P > 0 step inside the device loop's captured graph against direct launches, 200 vector steps, twice."""
    model = model_of("planar3", initial_joint_positions=[0.0, THETA - 0.05, 1.5 * np.pi - THETA], consider_autocollision=True)
    assert model.self_pairs == [(1, 3)]
    a, b, c = _loop_run(model, True), _loop_run(model, True), _loop_run(model, False)
    assert a == b
    assert a == c
    rf = len(a[1]) // 4 // 64
    rows = np.frombuffer(a[3], np.float32).reshape(-1, rf)
    _, off_r, _, _ = O.row_offsets(model.state_size, model.A)
    assert np.sum(rows[:, off_r] == -1000.0) >= 100                           # (the obstacle is out of the arm's plane: self-contacts)
    more = model_of("long12", consider_autocollision=True)                    # 55 pairs over 4 waves
    assert _loop_run(more, True, n=50) == _loop_run(more, False, n=50)


def test_many_capsules_take_fewer_envs_per_workgroup(tmp_path):
    """106 capsules need 159 KB of LDS for 64 envs: the launch takes 32 envs per workgroup (80 KB, above the 64 KB a kernel has
    unasked). Same bounds as the kernel-against-twin test, E = 100 so that the last workgroup is partly filled."""
    model = spiky_model(tmp_path, 34)
    twin = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), ORAD)
    tol = 16 * model.A * 2.0 ** -24 * model.reach
    E = 100
    far = np.float32([0.0, 0.0, 3.0 * model.reach]).astype(np.float64)
    rig = Rig(model, E, far, -far)
    tally = Tally()
    rng = np.random.default_rng(2)
    for _ in range(30):
        q = rng.uniform(-3.1416, 3.1416, (E, 3)).astype(np.float32)
        put(rig, q=q)
        got = probe(rig)
        check(rig, twin, q.astype(np.float64), np.broadcast_to(far, (E, 3)), np.broadcast_to(-far, (E, 3)), tol, tally, got,
              rig.step(np.zeros((E, 3), np.float32)))
    rig.close()
    print(f"spiky: steps {tally.steps} skipped {tally.skipped} self-contact only {tally.self_only} nothing {tally.nothing}")
    assert tally.skipped <= 0.01 * tally.steps and min(tally.self_only, tally.nothing) >= 100


def test_selfcol_end_to_end_and_resume(tmp_path):
    """initialize_kinematic_environment(consider_autocollision=True) -> run_training on 64 device envs: rows with reward -1000
    exist whose obstacle clearance, recomputed by the twin from the row's next state, is far from contact and whose self-clearance
    is negative (within the kernel-against-twin band of 0 at worst). A fresh process resumes bit-equal; the same arm with the
    option off is refused."""
    from chain_resume_worker import make_framework
    arm = near_contact_planar3()
    old = os.getcwd()
    try:
        os.makedirs(tmp_path / "full")
        os.chdir(tmp_path / "full")
        f = make_framework(arm)
        model = f.env.model
        assert model.self_pairs == [(1, 3)]
        full = f.run_training(1920, 30, verbose=False, n_envs=64)
        d_full = {k: str(v) for k, v in f.naf_agent.training_state_digest().items()}
        S, A = model.state_size, model.A
        _, off_r, off_s2, off_d = O.row_offsets(S, A)
        rows = f.naf_agent.memory.rows.cpu().numpy()
        rows = rows[np.any(rows != 0.0, axis=1)]
        assert len(rows) >= 200 * 64                                          # a few hundred vector steps
        hit = rows[rows[:, off_r] == -1000.0]
        assert len(hit) >= 100 and np.all(hit[:, off_d] == 1.0)
        twin = KinematicEnvironment(model, arm["target_position"], arm["obstacle_position"], ORAD)
        q = hit[:, off_s2:off_s2 + A].astype(np.float64)
        tol = 16 * A * 2.0 ** -24 * model.reach
        assert np.all(twin.clearance(q, hit[:, off_s2 + 2 * A + 6:off_s2 + 2 * A + 9].astype(np.float64)) > 1.0)
        sc = twin.self_clearance(q)
        assert np.all(sc < 4 * tol) and np.sum(sc < -4 * tol) >= 100
        free = rows[rows[:, off_r] != -1000.0]
        assert np.all(twin.self_clearance(free[:, off_s2:off_s2 + A].astype(np.float64)) > -4 * tol)
        out = str(tmp_path / "out.json")
        job = dict(cwd=str(tmp_path / "full"), arm=arm, episode=64, episodes=1920, frames=30, n_envs=64, out=out)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_resume_worker.py"), json.dumps(job)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        got = json.load(open(out))
        assert got["scores"] == {str(k): list(v) for k, v in full.items()}
        assert got["digests"] == d_full
        other = make_framework(near_contact_planar3(consider_autocollision=False), save=False)
        assert other.env.model.digest() != model.digest()
        with pytest.raises(ValueError, match="chain"):
            other.resume_training(64, 1920, 30, verbose=False, n_envs=64)
    finally:
        os.chdir(old)
