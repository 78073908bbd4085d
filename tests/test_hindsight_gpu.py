"""GPU (`-m gpu`): hindsight goals in the replay gather — naf_replay_gather_rows_hindsight against the float64 twin on synthetic
rings, the episode tag of naf_chain_env_step_tagged, the tagged loop with a relabelling chunk (graph and direct launches), the
framework's run / resume / refusals, and "off means off"."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chain_cell_common as K
from conftest import ROOT
from hindsight_common import (COUNTER, ENVS, HORIZONS, Ring, N_BATCHES, RATIOS, ROWS_PER_BATCH, SEED, SHAPES, case_indices, compare_with_twin,
                              gather_widths, hindsight_draw, synthetic_ring, twin_case)
from oracle import naf_oracle as O
from test_chain_env_cpu import model_of, path
from test_chain_env_gpu import _agent, scratch_cwd  # noqa: F401  (scratch_cwd is a fixture)

from robotic_manipulator_rloa_amd.utils import hindsight as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PLANAR = dict(manipulator_file=path("planar3"), endeffector_index=2, fixed_joints=[], involved_joints=[0, 1, 2],
              target_position=[0.45, 0.25, 0.0], obstacle_position=[0.1, -0.4, 0.3], initial_joint_positions=[0.3, -0.4, 0.5],
              initial_positions_variation_range=[0.1, 0.1, 0.1], link_radius=0.03, target_range=[0.15, 0.15, 0.0])


class RingRig:
    """A synthetic ring on the device behind a replay handle, driven through the C ABI directly."""

    def __init__(self, ring):
        from robotic_manipulator_rloa_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.ring = ring
        self.rows = torch.from_numpy(ring.phys.copy()).to(DEV)
        self.meta = torch.tensor([ring.head, ring.size, 123456, 0, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
        self.h = ctypes.c_void_p()
        assert self.lib.naf_replay_create(ring.capacity, ring.S, ring.A, self.rows.data_ptr(), self.meta.data_ptr(), ctypes.byref(self.h)) == 0
        # the sampler's counter as UpdateChunk leaves it (advanced past the chunk's minibatches), and the offset back to minibatch 0
        self.ctr = torch.tensor([COUNTER + N_BATCHES], dtype=torch.int64, device=DEV)
        self.off = (1 << 64) - N_BATCHES
        self.stream = torch.cuda.current_stream().cuda_stream

    def plain(self, idx, ld, mode=0):
        out = torch.full((idx.numel(), ld), 7.0, device=DEV)
        assert self.lib.naf_replay_gather_rows(self.h, idx.data_ptr(), out.data_ptr(), idx.numel(), ld, mode, self.stream) == 0
        return out.cpu().numpy()

    def descriptor(self, horizon, ratio, k_out, stride=None, **over):
        d = dict(stride=self.ring.E if stride is None else stride, horizon=horizon, ratio=ratio, rows_per_batch=ROWS_PER_BATCH,
                 seed=SEED, counter_dev=self.ctr.data_ptr(), counter_off=self.off, tag_col=self.ring.rf - 1,
                 k_out=None if k_out is None else k_out.data_ptr(), k0_out=None)
        d.update(over)
        return self._lib.Hindsight(**d)

    def hindsight(self, idx, ld, horizon, ratio, mode=0, want_k=True, **over):
        out = torch.full((idx.numel(), ld), 7.0, device=DEV)
        k = torch.full((idx.numel(),), -9, dtype=torch.int32, device=DEV) if want_k else None
        d = self.descriptor(horizon, ratio, k, **over)
        rc = self.lib.naf_replay_gather_rows_hindsight(self.h, idx.data_ptr(), out.data_ptr(), idx.numel(), ld, mode, ctypes.byref(d),
                                                       self.stream)
        assert rc == 0, rc
        return out.cpu().numpy(), (k.cpu().numpy() if want_k else None)

    def bad(self):
        return int(self.meta[7].item())

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_replay_destroy(self.h) == 0


@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("S,A", SHAPES)
def test_kernel_against_twin(S, A, E):
    """Every case of hindsight_common.cases() for this ring: H in {1, 8, 64, 1024} x ratio in {0, 0.5, 1}, n = 3 x 100 indices that
    hold the oldest and the newest rows, at every width of gather_widths. k_out exact; goal columns bit-equal; untouched columns
    bit-equal to naf_replay_gather_rows on the same idx; outside the band |d - 0.05| < 1e-6 done exact and reward within 1e-5 of
    the float64 twin; at most 1 % of the relabelled rows in the band; ratio 0 whole rows byte-equal to the plain gather."""
    ring = synthetic_ring(S, A, E)
    rig = RingRig(ring)
    idx_np = case_indices(ring.size)
    idx = torch.from_numpy(idx_np.copy()).to(DEV)
    for ld in gather_widths(S, A):
        plain = rig.plain(idx, ld)
        assert plain[:, :S].tobytes() == ring.deque[idx_np][:, :S].tobytes() and np.any(plain[:, S:S + A] != ring.deque[idx_np][:, S:S + A])
        for horizon in HORIZONS:
            for ratio in RATIOS:
                _, _, _, _, want_rows, want_k = twin_case(S, A, E, horizon, ratio)
                got_rows, got_k = rig.hindsight(idx, ld, horizon, ratio)
                if ratio == 0.0:
                    assert got_rows.tobytes() == plain.tobytes() and np.all(got_k == -1)
                    continue
                n_rel = compare_with_twin(ring, idx_np, want_rows[:, :ld], want_k, got_rows, got_k, plain)
                assert n_rel >= 30
                print(f"S={S} A={A} E={E} ld={ld} H={horizon} ratio={ratio}: relabelled {n_rel}, none valid {int(np.sum(want_k == -2))}")
    # float actions, no k_out, a NULL counter: the same rows under the other action mode; the draw at position counter_off alone
    ld = H.batch_row_floats(S, A)
    got, none = rig.hindsight(idx, ld, 8, 0.5, mode=1, want_k=False)
    assert none is None and got[:, S:S + A].tobytes() == ring.deque[idx_np][:, S:S + A].tobytes()
    got, k = rig.hindsight(idx, ld, 8, 0.5, counter_dev=None, counter_off=77)
    u, k0 = hindsight_draw(SEED, 77, idx_np.size, ROWS_PER_BATCH, 8)
    assert np.array_equal(k, H.relabel_rows(ring.deque, idx_np, u, k0, E, 8, 0.5, S, A)[1])
    assert rig.bad() == 0
    rig.close()


def test_bad_indices_and_argument_errors():
    ring = synthetic_ring(23, 7, 3)
    rig = RingRig(ring)
    idx_np = case_indices(ring.size).copy()
    idx_np[5], idx_np[150] = -1, ring.size
    idx = torch.from_numpy(idx_np).to(DEV)
    plain = rig.plain(idx, 56)
    assert rig.bad() == 2
    got, k = rig.hindsight(idx, 56, 8, 1.0)
    assert rig.bad() == 4 and k[5] == -1 and k[150] == -1
    assert got[[5, 150]].tobytes() == plain[[5, 150]].tobytes()            # row 0, as the plain gather writes it
    out = torch.zeros(4, 56, device=DEV)

    def rc(ld=56, n=4, **over):
        d = rig.descriptor(over.pop("horizon", 8), over.pop("ratio", 0.5), None, **over)
        return rig.lib.naf_replay_gather_rows_hindsight(rig.h, idx.data_ptr(), out.data_ptr(), n, ld, 0, ctypes.byref(d), rig.stream)
    assert rc() == 0 and rc(n=0) == 0
    for over in (dict(stride=0), dict(horizon=0), dict(horizon=1025), dict(ratio=-0.5), dict(ratio=1.5), dict(ratio=float("nan")),
                 dict(rows_per_batch=0), dict(tag_col=55), dict(tag_col=64), dict(counter_dev=rig.ctr.data_ptr() + 4)):
        assert rc(**over) == -1, over
    assert rc(ld=54) == -1 and rc(ld=52) == -1 and rc(ld=68) == -1 and rc(n=-1) == -1
    assert rig.lib.naf_replay_gather_rows_hindsight(rig.h, idx.data_ptr(), out.data_ptr(), 4, 56, 0, None, rig.stream) == -1
    assert rig.bad() == 4
    rig.close()
    # a ring of another row layout (S != 2 A + 9) is refused
    rows = torch.zeros(8, 64, device=DEV)
    meta = torch.zeros(8, dtype=torch.int64, device=DEV)
    h = ctypes.c_void_p()
    assert rig.lib.naf_replay_create(8, 21, 7, rows.data_ptr(), meta.data_ptr(), ctypes.byref(h)) == 0
    d = rig.descriptor(8, 0.5, None)
    assert rig.lib.naf_replay_gather_rows_hindsight(h, idx.data_ptr(), out.data_ptr(), 4, 56, 0, ctypes.byref(d), rig.stream) == -1
    assert rig.lib.naf_replay_destroy(h) == 0
    # the host wrapper refuses before any launch
    from robotic_manipulator_rloa_amd.utils.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(100, 4, DEV, 0, state_size=23, action_size=7)
    o4, i4 = torch.zeros(4, 56, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    for kw, what in ((dict(ratio=1.5), "ratio"), (dict(horizon=0), "horizon"), (dict(stride=0), "stride"), (dict(rows_per_batch=0), "stride")):
        with pytest.raises(ValueError, match=what):
            rb.gather_rows_hindsight(i4, o4, 4, **dict(dict(stride=1, horizon=8, ratio=0.5, rows_per_batch=4, counter_off=0), **kw))
    with pytest.raises(ValueError, match="int32"):
        rb.gather_rows_hindsight(i4, o4, 4, 1, 8, 0.5, 4, 0, k_out=torch.zeros(4, device=DEV))
    with pytest.raises(ValueError, match="21 joints"):
        ReplayBuffer(100, 4, DEV, 0, state_size=51, action_size=21).gather_rows_hindsight(i4, o4, 4, 1, 8, 0.5, 4, 0)


# ---- the tagged step ---------------------------------------------------------------------------------------------------------------
class StepRig:
    """E device envs of one chain model through the C ABI, stepped by naf_chain_env_step or naf_chain_env_step_tagged."""
    K = 4

    def __init__(self, model, E, ranges, tagged):
        from robotic_manipulator_rloa_amd import _lib
        self.lib = _lib.load()
        self.E, self.A, self.S, self.tagged = E, model.A, model.state_size, tagged
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        self.rf = self.lib.naf_replay_row_floats(self.S, self.A)
        self.st = torch.zeros(E, self.lib.naf_chain_env_state_floats(self.h), device=DEV)
        self.obs = torch.zeros(E, self.S, device=DEV)
        self.rows = torch.full((E, self.rf), 7.0, device=DEV)
        self.ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.recs = torch.zeros(self.K, E, 8, dtype=torch.int32, device=DEV)
        self.stream = torch.cuda.current_stream().cuda_stream
        if ranges is not None:
            assert self.lib.naf_chain_env_set_scene_ranges(self.h, (ctypes.c_float * 7)(*ranges)) == 0
        ee = model.reach * np.array([0.5, 0.3, 0.2])
        scene = (ctypes.c_float * 8)(*[float(v) for v in ee], *[float(v) for v in 0.6 * ee], 0.0, 0.06)
        assert self.lib.naf_chain_env_reset(self.h, self.st.data_ptr(), self.obs.data_ptr(), E, scene, 5, 0, self.stream) == 0

    def step(self, actions, max_frames):
        a_d = torch.from_numpy(np.ascontiguousarray(actions, np.float32)).to(DEV)
        fn = self.lib.naf_chain_env_step_tagged if self.tagged else self.lib.naf_chain_env_step
        assert fn(self.h, self.st.data_ptr(), a_d.data_ptr(), self.rows.data_ptr(), self.obs.data_ptr(), self.E, 5, self.ctr.data_ptr(),
                  max_frames, self.recs.data_ptr(), self.K, self.stream) == 0
        t = int(self.ctr.item())
        assert self.lib.naf_counter_add(self.ctr.data_ptr(), 1, self.stream) == 0
        return self.rows.cpu().numpy(), self.st.cpu().numpy(), self.obs.cpu().numpy(), self.recs[t % self.K].cpu().numpy()

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


def _step_models():
    return {"planar3": (lambda: model_of("planar3"), None),
            "iiwa_like7-selfcol": (lambda: model_of("iiwa_like7", consider_autocollision=True), None),
            "iiwa_like7-ranges": (lambda: model_of("iiwa_like7"), (0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.02)),
            "iiwa_like7-workcell": (lambda: K.arm("iiwa_like7")[0], None),
            "planar3-workcell-ranges": (lambda: K.arm("planar3")[0], (0.1, 0.1, 0.0, 0.05, 0.05, 0.0, 0.02)),
            # the tagged instantiations the five above leave out: pairs with ranges, a workcell without pairs, all three together
            "iiwa_like7-selfcol-ranges": (lambda: model_of("iiwa_like7", consider_autocollision=True), (0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.02)),
            "planar3-workcell": (lambda: K.arm("planar3")[0], None),
            "iiwa_like7-workcell-ranges": (lambda: K.arm("iiwa_like7")[0], (0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.02))}


@pytest.mark.parametrize("E", [1, 64, 100])
@pytest.mark.parametrize("name", list(_step_models()))
def test_tagged_step(name, E):
    """max_frames = 2, 20 steps of N(0, 1) actions from the same state through both entries: every row's last float equals the
    `episode` of that step's record; every other float of the row, env_state, obs_next and the records are bit-equal."""
    from robotic_manipulator_rloa_amd.engine import EPISODE_RECORD
    make, ranges = _step_models()[name]
    model = make()
    plain, tagged = StepRig(model, E, ranges, False), StepRig(model, E, ranges, True)
    rng = np.random.default_rng(1)
    seen = set()
    for t in range(20):
        act = rng.normal(size=(E, model.A)).astype(np.float32)
        a, b = plain.step(act, 2), tagged.step(act, 2)
        episode = b[3].view(EPISODE_RECORD).reshape(E)["episode"]
        assert np.array_equal(b[0][:, -1], episode.astype(np.float32)) and np.all(a[0][:, -1] == 0)
        assert a[0][:, :-1].tobytes() == b[0][:, :-1].tobytes()
        for x, y in zip(a[1:], b[1:]):
            assert x.tobytes() == y.tobytes()
        seen |= set(episode.tolist())
    assert seen >= set(range(1, 10))           # episodes turned over: at least every second step
    plain.close()
    tagged.close()


def test_tagged_step_refuses_an_arm_without_a_spare_float():
    """A = 8 (standin8): the minibatch row takes all 64 floats of the ring row"""
    model = model_of("standin8")
    assert H.tag_column(model.state_size, model.A) is None
    rig = StepRig(model, 4, None, True)
    a_d = torch.zeros(4, model.A, device=DEV)
    args = (rig.h, rig.st.data_ptr(), a_d.data_ptr(), rig.rows.data_ptr(), rig.obs.data_ptr(), 4, 5, rig.ctr.data_ptr(), 2, None, 0, rig.stream)
    assert rig.lib.naf_chain_env_step_tagged(*args) == -1 and rig.lib.naf_chain_env_step(*args) == 0
    rig.close()
    from robotic_manipulator_rloa_amd.engine import DeviceEnvLoop, UpdateChunk
    agent = _agent(model)
    with pytest.raises(ValueError, match="8 joints"):
        DeviceEnvLoop(agent.learner, agent.memory, 8, seed=1, chain=model, target=(0.3, 0.2, 0.6), obstacle=(0.2, 0.1, 0.4), tag_rows=True)
    with pytest.raises(ValueError, match="8 joints"):
        UpdateChunk(agent.learner, agent.memory, 2, hindsight=(0.5, 8, 8))
    with pytest.raises(ValueError, match="stand-in"):
        DeviceEnvLoop(agent.learner, agent.memory, 8, seed=1, tag_rows=True)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
def _loop_scenario(use_graph):
    """DeviceEnvLoop(tag_rows=True) + UpdateChunk(hindsight=(0.8, 8, 64)) on planar3, E = 64, B = 64, U = 2, 40 vector steps; after
    each of the last 5 steps: (ring in deque order, idx, stream position of minibatch 0, batch, k_out, k0_out, plain gather)."""
    from robotic_manipulator_rloa_amd.engine import DeviceEnvLoop, UpdateChunk
    model = model_of("planar3")
    agent = _agent(model)
    mem = agent.memory
    loop = DeviceEnvLoop(agent.learner, mem, 64, seed=9, max_frames=6, use_graph=use_graph, chain=model, target=(0.45, 0.25, 0.0),
                         obstacle=(0.1, -0.4, 0.3), target_range=[0.15, 0.15, 0.0], tag_rows=True)
    chunk = UpdateChunk(agent.learner, mem, 2, use_graph=use_graph, hindsight=(0.8, 8, 64))
    seen = []
    plain = torch.zeros_like(chunk.batch)
    for t in range(40):
        loop.step()
        if len(mem) > 64:
            chunk.run()
        if t >= 35:
            torch.cuda.synchronize()
            mem.gather_rows(chunk.idx, plain, 128)
            size = int(mem.meta[1].item())
            assert size == 64 * (t + 1) and int(mem.meta[0].item()) == size          # not wrapped: deque order is memory order
            seen.append((mem.rows[:size].cpu().numpy(), chunk.idx.cpu().numpy().reshape(-1), int(mem._sample_ctr.item()) - 2,
                         chunk.batch.cpu().numpy().reshape(128, -1), chunk.k_out.cpu().numpy().reshape(-1),
                         chunk.k0_out.cpu().numpy().reshape(-1), plain.cpu().numpy().reshape(128, -1), mem.seed))
    torch.cuda.synchronize()
    return seen, agent.learner.theta2.cpu().numpy().tobytes()


def test_loop_against_twin_and_graph_equals_direct_launches():
    model = model_of("planar3")
    S, A = model.state_size, model.A
    ring = Ring()          # carries the loop's own rows to compare_with_twin
    ring.S, ring.A, ring.E = S, A, 64
    graph, direct = _loop_scenario(True), _loop_scenario(False)
    relabelled = 0
    for rows, idx, pos, batch, k, k0_dev, plain, seed in graph[0]:
        ring.deque = rows
        assert np.all(rows[:, -1] >= 1) and rows[:, -1].max() >= 4      # tagged, and episodes turned over
        u, k0 = hindsight_draw(seed, pos, 128, 64, 8)
        want_rows, want_k = H.relabel_rows(rows, idx, u, k0, 64, 8, 0.8, S, A)
        relabelled += compare_with_twin(ring, idx, want_rows[:, :batch.shape[1]], want_k, batch, k, plain)
        assert np.array_equal(k0_dev, np.where(want_k == -1, -1, k0))
    assert relabelled >= 5 * 128 * 0.5
    for a, b in zip(graph[0], direct[0]):
        for x, y in zip(a[:7], b[:7]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert graph[1] == direct[1]


# ---- the framework -----------------------------------------------------------------------------------------------------------------
def test_framework_run_resume_and_refusals(tmp_path):
    """512 episodes of at most 20 frames on 64 envs, drains every 64 vector steps: the drain at step 64 writes checkpoint 64 and the
    run goes on for two more drains, so the resumed process trains 128 vector steps of its own before the digests are compared."""
    from chain_resume_worker import make_framework
    old = os.getcwd()
    try:
        os.makedirs(tmp_path / "full")
        os.chdir(tmp_path / "full")
        f = make_framework(PLANAR)
        full = f.run_training(512, 20, verbose=False, n_envs=64, hindsight=0.8)
        stats = f.naf_agent.last_run_stats
        assert {"hindsight_relabelled_share", "hindsight_shortened_share", "hindsight_reached_share"} <= set(stats)
        assert 0.3 < stats["hindsight_relabelled_share"] <= 1.0 and 0.0 <= stats["hindsight_reached_share"] <= 1.0
        print({k: v for k, v in stats.items() if k.startswith("hindsight")})
        mem = f.naf_agent.memory
        assert np.all(mem.rows[:len(mem), -1].cpu().numpy() >= 1)
        d_full = {k: str(v) for k, v in f.naf_agent.training_state_digest().items()}
        st = torch.load("checkpoints/64/training_state.pt", weights_only=True)
        args = st["sections"]["loop"]["meta"]["args"]
        assert args["hindsight"] == 0.8 and args["hindsight_horizon"] == 20
        out = str(tmp_path / "out.json")
        job = dict(cwd=str(tmp_path / "full"), arm=PLANAR, episode=64, episodes=512, frames=20, n_envs=64, hindsight=0.8, out=out)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hindsight_resume_worker.py"), json.dumps(job)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        got = json.load(open(out))
        assert got["scores"] == {str(k): list(v) for k, v in full.items()}
        assert got["digests"] == d_full
        # another ratio, another horizon, or none, are refused through the comparison of the saved arguments
        for kw in (dict(hindsight=0.5), dict(hindsight=0.8, hindsight_horizon=10), dict()):
            other = make_framework(PLANAR, save=False)
            with pytest.raises(ValueError, match="hindsight"):
                other.resume_training(64, 512, 20, verbose=False, n_envs=64, **kw)
        # a ring with foreign rows; the one-env loop
        foreign = make_framework(PLANAR, save=False)
        S, A = foreign.env.model.state_size, foreign.env.model.A
        foreign.naf_agent.memory.add(np.zeros(S, np.float32), np.zeros(A, np.float32), 0.0, np.zeros(S, np.float32), 0)
        with pytest.raises(ValueError, match="already holds 1 rows"):
            foreign.run_training(4, 20, verbose=False, n_envs=64, hindsight=0.8)
        with pytest.raises(ValueError, match="n_envs > 1"):
            foreign.run_training(4, 20, verbose=False, hindsight=0.8)
    finally:
        os.chdir(old)


def test_hindsight_off_is_the_call_without_the_arguments(scratch_cwd):  # noqa: F811
    from robotic_manipulator_rloa_amd import training_state
    model = model_of("planar3")
    scene = {"target": [0.45, 0.25, 0.0], "obstacle": [0.1, -0.4, 0.3], "target_range": [0.15, 0.15, 0.0]}
    states = []
    for kw in ({}, dict(hindsight=0.0), dict(hindsight=0.0, hindsight_horizon=16)):
        agent = _agent(model)
        out = agent.run_vectorized(30, n_envs=64, max_frames=8, drain_every=8, chain=model, scene=scene, **kw)
        assert out["updates"] > 0 and not any(k.startswith("hindsight") for k in out)
        rows = agent.memory.rows[:len(agent.memory)].cpu().numpy()
        off_d = O.row_offsets(model.state_size, model.A)[3]
        assert rows.shape[0] == 30 * 64 and np.all(rows[:, off_d + 1:] == 0)
        sec = training_state.collect(agent)
        states.append(b"".join(sec[s]["tensors"][k].cpu().numpy().tobytes() for s in ("learner", "replay", "actor")
                               for k in sorted(sec[s]["tensors"])))
    assert states[0] == states[1] and states[0] == states[2]
