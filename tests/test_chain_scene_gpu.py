"""GPU (`-m gpu`): a new target and obstacle every episode (csrc/chain_env.hip, SCENE = true) — reset and auto-reset against the
float64 twin's choose_scene, "off means off", determinism, the kinematic environment with ranges end to end, and resume."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chain_scene_common import CASES, MARGIN, ORAD, find_boxes, run_arm
from conftest import ROOT
from test_chain_env_cpu import model_of
from test_chain_env_gpu import DEV, IIWA, Rig, _agent, scratch_cwd  # noqa: F401  (scratch_cwd is a fixture)

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -2


class SceneRig(Rig):
    """test_chain_env_gpu.Rig with scene ranges: they are set after the handle exists, then the envs are reset under them."""

    def __init__(self, model, E, boxes, seed, record_slots=0):
        tc, tr, oc, orr = boxes
        super().__init__(model, E, tc, oc, orad=ORAD, seed=seed, record_slots=record_slots)
        self.ranges = (ctypes.c_float * 7)(*[float(v) for v in tr], *[float(v) for v in orr], MARGIN)
        assert self.lib.naf_chain_env_set_scene_ranges(self.h, self.ranges) == 0
        self.reset()

    def reset(self):
        assert self.lib.naf_chain_env_reset(self.h, self.st.data_ptr(), self.obs.data_ptr(), self.E, self.scene, self.seed, 0,
                                            self.stream) == 0
        self.ctr.zero_()

    def read(self):
        return self.st.cpu().numpy(), self.obs.cpu().numpy()

    def everything(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().tobytes() for t in (self.st, self.obs, self.rows) + ((self.recs,) if self.recs is not None else ()))


@pytest.mark.parametrize("E", [1, 64, 100])
@pytest.mark.parametrize("name,autocollision", CASES)
def test_reset_and_auto_reset_against_the_twin(name, autocollision, E):
    """max_frames = 2, N(0, 1) actions, 100 steps, in a loose and a tight scene (chain_scene_common.find_boxes). After the reset and
    after every step, for each env whose episode count rose: the K candidates restated from Philox with `ctr` as the kernel forms
    it, fed with the kernel's own q0 to choose_scene; target and obstacle equal, bit for bit, the float64 expression rounded once to
    float32; obs_next's slots equal env_state's; the finished row's next_state holds the previous scene; the other envs keep theirs.
    A draw is skipped when a margin of a candidate at or before the twin's choice lies within 2 tol of its threshold, tol =
    16 A 2^-24 reach — at most 1 % of the case's draws; the case is vacuous unless the twin alone counts >= 30 draws that take
    candidate 0, take a later one, are rejected by condition 1, 2, 3, and fall back (loose and tight summed)."""
    total = run_arm(name, autocollision, E, lambda model, boxes, seed: SceneRig(model, E, boxes, seed))
    print(f"{name} E={E}: {total}")


def _rollout(rig, steps, max_frames, seed=3):
    rng = np.random.default_rng(seed)
    out = [rig.everything()]
    for _ in range(steps):
        rig.step(rng.normal(size=(rig.E, rig.A)).astype(np.float32), max_frames=max_frames)
        out.append(rig.everything())
    return out


@pytest.mark.parametrize("name,autocollision", [("planar3", False), ("iiwa_like7", True)])
def test_off_means_off(name, autocollision):
    model = model_of(name, consider_autocollision=autocollision)
    E, K = 100, 8
    tc, tr, oc, orr = find_boxes(model, "tight")          # the nominal obstacle touches the arm: episodes end by contact too

    def rig_with(ranges):
        rig = Rig(model, E, tc, oc, orad=ORAD, seed=5, record_slots=K)
        rig.everything = SceneRig.everything.__get__(rig)
        if ranges != "never":
            assert rig.lib.naf_chain_env_set_scene_ranges(rig.h, ranges) == 0
            SceneRig.reset(rig)
        return rig
    rigs = [rig_with("never"), rig_with((ctypes.c_float * 7)(*([0.0] * 6), 0.02)), rig_with(None)]
    runs = [_rollout(r, 50, 3) for r in rigs]
    assert runs[0] == runs[1] and runs[0] == runs[2]
    st = rigs[0].st.cpu().numpy()
    assert st[:, model.A + 8].min() >= 50 // 3 and np.all(st[:, model.A:model.A + 3] == np.float32(tc))
    # the documented codes, and a handle that refused its ranges stays as it was
    r = rigs[1]
    for bad in ([0.1, -0.1, 0, 0, 0, 0, 0.02], [0.1, float("nan"), 0, 0, 0, 0, 0.02], [0.1, 0, 0, 0, 0, 0, -0.02],
                [float("inf"), 0, 0, 0, 0, 0, 0.02]):
        assert r.lib.naf_chain_env_set_scene_ranges(r.h, (ctypes.c_float * 7)(*bad)) == ERR_ARG
    assert r.lib.naf_chain_env_set_scene_ranges(None, None) == ERR_ARG
    r.step(np.zeros((E, model.A), np.float32), max_frames=3)
    assert r.lib.naf_chain_env_set_scene_ranges(r.h, (ctypes.c_float * 7)(0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.02)) == 0
    a_d = torch.zeros(E, model.A, device=DEV)
    step = lambda: r.lib.naf_chain_env_step(r.h, r.st.data_ptr(), a_d.data_ptr(), r.rows.data_ptr(), r.obs.data_ptr(), E, r.seed,  # noqa: E731
                                            r.ctr.data_ptr(), 3, None, 0, r.stream)
    assert step() == ERR_STATE                               # ranges set and no reset since
    jitter = (ctypes.c_float * 8)(*[float(v) for v in tc], *[float(v) for v in oc], 0.05, ORAD)
    assert r.lib.naf_chain_env_reset(r.h, r.st.data_ptr(), r.obs.data_ptr(), E, jitter, 5, 0, r.stream) == ERR_ARG
    assert step() == ERR_STATE
    SceneRig.reset(r)
    assert step() == 0
    assert r.lib.naf_chain_env_set_scene_ranges(r.h, None) == 0      # cleared: the jitter is welcome again
    assert r.lib.naf_chain_env_reset(r.h, r.st.data_ptr(), r.obs.data_ptr(), E, jitter, 5, 0, r.stream) == 0
    for x in rigs:
        x.close()


def test_same_seed_same_bits():
    model = model_of("iiwa_like7", consider_autocollision=True)
    boxes = find_boxes(model, "loose")
    a, b, c = (_rollout(SceneRig(model, 100, boxes, seed, record_slots=8), 40, 3) for seed in (5, 5, 6))
    assert a == b and a != c
    assert a[0][0] != a[-1][0]


RANGES = dict(target_range=[0.15, 0.15, 0.1], obstacle_range=[0.1, 0.1, 0.1])


def _loop_run(model, use_graph, n=120):
    from robotic_manipulator_rloa_amd.engine import DeviceEnvLoop
    agent = _agent(model)
    loop = DeviceEnvLoop(agent.learner, agent.memory, 64, seed=9, max_frames=10, use_graph=use_graph, records=True, drain_every=8,
                         chain=model, target=(0.45, 0.3, 0.6), obstacle=(0.35, 0.2, 0.45), scene_margin=0.02, **RANGES)
    assert loop.scene[8:] == RANGES["target_range"] + RANGES["obstacle_range"] + [0.02] and len(loop.scene) == 15
    for _ in range(n):
        loop.step()
    episodes = loop.drain(final=True)
    torch.cuda.synchronize()
    return (loop.env_state.cpu().numpy().tobytes(), loop.rows.cpu().numpy().tobytes(), loop.records.cpu().numpy().tobytes(),
            agent.memory.rows[:n * 64].cpu().numpy().tobytes(), episodes)


def test_graph_equals_direct_launches_with_ranges():
    from robotic_manipulator_rloa_amd.engine import DeviceEnvLoop
    model = model_of("iiwa_like7")
    a, c = _loop_run(model, True), _loop_run(model, False)
    assert a == c and len(a[4]) >= 64 * (120 // 10)
    A = model.A
    targets = np.frombuffer(a[3], np.float32).reshape(120 * 64, -1)[:, 2 * A + 3:2 * A + 6]
    assert len({t.tobytes() for t in targets}) >= 64 * (120 // 10)
    # a loop without ranges keeps exactly the scene it had; jitter and ranges exclude each other
    agent = _agent(model)
    plain = DeviceEnvLoop(agent.learner, agent.memory, 8, seed=9, chain=model, target=(0.45, 0.3, 0.6), obstacle=(0.35, 0.2, 0.45),
                          target_range=[0, 0, 0])
    assert len(plain.scene) == 8
    with pytest.raises(ValueError, match="exclude"):
        DeviceEnvLoop(agent.learner, agent.memory, 8, seed=9, chain=model, target=(0.45, 0.3, 0.6), obstacle=(0.35, 0.2, 0.45),
                      obstacle_jitter=0.01, **RANGES)


def _in_boxes(rows, A):
    tc, oc = np.float32(IIWA["target_position"]), np.float32(IIWA["obstacle_position"])
    tr, orr = np.float32(RANGES["target_range"]), np.float32(RANGES["obstacle_range"])
    t, o = rows[:, 2 * A + 3:2 * A + 6], rows[:, 2 * A + 6:2 * A + 9]
    eps = np.float32(1e-6)
    return bool(np.all(np.abs(t - tc) <= tr + eps) and np.all(np.abs(o - oc) <= orr + eps))


def test_kinematic_environment_with_ranges_end_to_end(scratch_cwd):  # noqa: F811
    from chain_resume_worker import make_framework
    f = make_framework(dict(IIWA, **RANGES), checkpoint_frequency=64, save=False)
    scores = f.run_training(6, 40, verbose=False, n_envs=64)
    assert list(scores.keys()) == list(range(1, 7))
    assert all(np.isfinite(s) and 0 <= fr <= 40 for s, fr in scores.values())
    assert os.path.isfile("model.p")
    out = f.test_trained_model(16, 40, n_envs=16)
    assert set(out) == {"successes", "episodes", "collisions", "mean_frames_to_success"} and out["episodes"] == 16
    assert 0 <= out["successes"] + out["collisions"] <= 16
    mem, A, S = f.naf_agent.memory, f.env.model.A, f.env.model.state_size
    rows = mem.rows[:len(mem)].cpu().numpy()
    assert rows.shape[0] >= 64 * 40
    assert len({r.tobytes() for r in rows[:, 2 * A + 3:2 * A + 6]}) >= 8
    off_s2 = -(-(S + A + 1) // 4) * 4
    assert _in_boxes(rows, A) and _in_boxes(rows[:, off_s2:], A)
    # one env on the host twin draws by the same rule
    one = f.run_training(2, 10, verbose=False)
    assert list(one.keys()) == [1, 2]
    one = f.test_trained_model(2, 10)
    assert one["episodes"] == 2


def test_resume_with_ranges_in_a_fresh_process(tmp_path):
    from chain_resume_worker import make_framework
    arm = dict(IIWA, **RANGES)
    old = os.getcwd()
    try:
        os.makedirs(tmp_path / "full")
        os.chdir(tmp_path / "full")
        f = make_framework(arm)
        full = f.run_training(128, 20, verbose=False, n_envs=64)
        d_full = {k: str(v) for k, v in f.naf_agent.training_state_digest().items()}
        st = torch.load("checkpoints/64/training_state.pt", weights_only=True)
        scene = st["sections"]["loop"]["meta"]["args"]["scene"]
        assert len(scene) == 15 and scene[8:] == pytest.approx(RANGES["target_range"] + RANGES["obstacle_range"] + [0.02])
        assert scene[:3] == pytest.approx(IIWA["target_position"])          # the centres, not some episode's scene
        out = str(tmp_path / "out.json")
        job = dict(cwd=str(tmp_path / "full"), arm=arm, episode=64, episodes=128, frames=20, n_envs=64, out=out)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_scene_resume_worker.py"), json.dumps(job)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        got = json.load(open(out))
        assert got["scores"] == {str(k): list(v) for k, v in full.items()}
        assert got["digests"] == d_full
        # other ranges, or none, are refused by the scene comparison
        other = make_framework(dict(arm, target_range=[0.15, 0.15, 0.05]), save=False)
        with pytest.raises(ValueError, match="scene"):
            other.resume_training(64, 128, 20, verbose=False, n_envs=64)
        fixed = make_framework(IIWA, save=False)
        with pytest.raises(ValueError, match="scene"):
            fixed.resume_training(64, 128, 20, verbose=False, n_envs=64)
    finally:
        os.chdir(old)
