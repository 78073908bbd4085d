"""GPU (`-m gpu`): the workcell instantiations of csrc/chain_env.hip — naf_chain_env_probe_cell, the rollout step and the training
step with floor, walls and fixed spheres — against the float64 twin (environment/kinematic.py) through the C ABI, the masks, that
nothing changes without a workcell, graph capture, and the kinematic environment with a workcell end to end."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

import chain_cell_common as K
import chain_rollout_common as C
from oracle import naf_oracle as O
from test_chain_env_cpu import ARMS as ARM_TABLE
from test_chain_env_cpu import model_of, path

from robotic_manipulator_rloa_amd.environment.kinematic import KinematicEnvironment
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = K.FRAMES


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class CellRig:
    """E device envs of one chain model, driven through the C ABI directly: training reset / step, given reset / rollout step and
    the two probes."""

    def __init__(self, model, E, frames=F, blob=None, ranges=None, record_slots=0, seed=5):
        from robotic_manipulator_rloa_amd import _lib
        self.lib = _lib.load()
        self.m, self.E, self.A, self.S, self.frames, self.seed = model, E, model.A, model.state_size, frames, seed
        blob = np.ascontiguousarray(model.pack() if blob is None else blob, np.float32)
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        if ranges is not None:
            assert self.lib.naf_chain_env_set_scene_ranges(self.h, (ctypes.c_float * 7)(*ranges)) == 0
        self.nst = self.lib.naf_chain_env_state_floats(self.h)
        self.rf = self.lib.naf_replay_row_floats(self.S, self.A)
        _, self.off_r, self.off_s2, self.off_d = O.row_offsets(self.S, self.A)
        z = dict(device=DEV)
        self.st, self.obs = torch.zeros(E, self.nst, **z), torch.zeros(E, self.S, **z)
        self.rows, self.out = torch.zeros(E, self.rf, **z), torch.zeros(E, 8, **z)
        self.traj = torch.zeros(frames + 1, E, self.A, **z)
        self.q0, self.scene, self.act = torch.zeros(E, self.A, **z), torch.zeros(E, 6, **z), torch.zeros(E, self.A, **z)
        self.ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.K = record_slots
        self.recs = torch.zeros(record_slots, E, 8, dtype=torch.int32, device=DEV) if record_slots else None

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def reset(self, target, obstacle, orad=K.ORAD):
        scene = (ctypes.c_float * 8)(*[float(v) for v in target], *[float(v) for v in obstacle], 0.0, orad)
        assert self.lib.naf_chain_env_reset(self.h, self.st.data_ptr(), self.obs.data_ptr(), self.E, scene, self.seed, 0, self.stream) == 0
        self.ctr.zero_()

    def reset_given(self, q0, target, obstacle):
        self.q0.copy_(torch.from_numpy(np.ascontiguousarray(q0, np.float32)))
        self.scene.copy_(torch.from_numpy(np.concatenate([target, obstacle], axis=1).astype(np.float32)))
        assert self.lib.naf_chain_env_reset_given(self.h, self.st.data_ptr(), self.obs.data_ptr(), self.E, self.q0.data_ptr(),
                                                  self.scene.data_ptr(), K.ORAD, self.stream) == 0

    def load_actions(self, actions):
        self.act.copy_(torch.from_numpy(np.ascontiguousarray(actions, np.float32)))

    def launch_step(self, max_frames=0):
        assert self.lib.naf_chain_env_step(self.h, self.st.data_ptr(), self.act.data_ptr(), self.rows.data_ptr(), self.obs.data_ptr(),
                                           self.E, self.seed, self.ctr.data_ptr(), max_frames,
                                           self.recs.data_ptr() if self.recs is not None else None, self.K, self.stream) == 0
        assert self.lib.naf_counter_add(self.ctr.data_ptr(), 1, self.stream) == 0

    def launch_rollout(self):
        assert self.lib.naf_chain_env_rollout_step(self.h, self.st.data_ptr(), self.act.data_ptr(), self.obs.data_ptr(),
                                                   self.out.data_ptr(), self.traj.data_ptr(), self.E, self.frames, self.stream) == 0

    def probe_cell(self):
        out = torch.full((self.E + 28,), float("nan"), device=DEV)             # (rows behind the E envs': no lane may write them)
        rc = self.lib.naf_chain_env_probe_cell(self.h, self.st.data_ptr(), out.data_ptr(), self.E, self.stream)
        out = out.cpu().numpy()
        assert np.all(np.isnan(out[self.E:]))
        return rc, out[:self.E]

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


# ---- (1) probe_cell ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.ARMS)
def test_probe_cell_against_twin(name):
    """256 uniform poses per arm: within 2 tol of cell_clearance, the sign equal outside |clearance| <= 2 tol (at most 1 % of the
    poses inside). naf_chain_env_probe's five floats are what they are on the arm without a workcell."""
    model, twin = K.arm(name)
    q = K.uniform_poses(name)
    n, tol = len(q), K.tol_of(model)
    far_t, far_o = C.away(model)
    rig = CellRig(model, n)
    rig.reset_given(q, np.tile(far_t, (n, 1)), np.tile(far_o, (n, 1)))
    rc, got = rig.probe_cell()
    five = torch.zeros(n, 5, device=DEV)
    assert rig.lib.naf_chain_env_probe(rig.h, rig.st.data_ptr(), five.data_ptr(), n, rig.stream) == 0
    assert rig.lib.naf_chain_env_probe_cell(rig.h, rig.st.data_ptr(), None, n, rig.stream) == -1
    rig.close()
    assert rc == 0
    want = twin.cell_clearance(q)
    err = np.abs(got - want)
    inside = np.abs(want) <= 2 * tol
    print(f"{name}: worst error {err.max():.2e} (2 tol = {2 * tol:.2e}), {int(inside.sum())} of {n} inside the band, "
          f"{int(np.sum(want < 0))} in contact")
    assert err.max() <= 2 * tol, (err.max(), tol)
    assert inside.sum() <= 0.01 * n and np.array_equal((got < 0)[~inside], (want < 0)[~inside])
    base = CellRig(K.plain(name), n)
    base.reset_given(q, np.tile(far_t, (n, 1)), np.tile(far_o, (n, 1)))
    five0 = torch.zeros(n, 5, device=DEV)
    assert base.lib.naf_chain_env_probe(base.h, base.st.data_ptr(), five0.data_ptr(), n, base.stream) == 0
    rc0, _ = base.probe_cell()
    base.close()
    assert rc0 == -2                                                       # NAF_ERR_STATE: the blob has no workcell
    assert bits(five.cpu().numpy()).tobytes() == bits(five0.cpu().numpy()).tobytes()


# ---- (2) rollout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", K.SIZES)
@pytest.mark.parametrize("name", K.ARMS)
def test_rollout_kernel_against_twin(name, E):
    """reset_given + 40 rollout steps with the case's scripted actions; the twin is evaluated at the RECORDED joint values
    (teacher-forced). Code, frames and outcome[6] are held to it: code and frames equal, except that an env is skipped from its
    first step inside the band (chain_cell_common.band4; at most 1 % of the (env, step) pairs, at least 8 envs per outcome
    compared to their end when E >= 64); outcome[6] within 2 tol of the minimum of the twin's workcell clearance over the same
    poses, outcome[3] within 2 tol of the obstacle's."""
    case = K.build_case(name, E)
    model, A, tol = case.model, case.model.A, K.tol_of(case.model)
    rig = CellRig(model, E)
    rig.reset_given(case.q0, case.target, case.obstacle)
    st0 = rig.st.cpu().numpy()
    for t in range(F):
        rig.load_actions(case.act[:, t])
        rig.launch_rollout()
    out, traj, st = rig.out.cpu().numpy(), rig.traj.cpu().numpy(), rig.st.cpu().numpy()
    rig.close()
    traj[0] = st0[:, :A]
    code, fd = out[:, 0].astype(np.int64), out[:, 1].astype(np.int64)
    assert np.all((fd >= 1) & (fd <= F)) and np.all(np.isin(code, (0, 1, 2, 3, 4))) and np.all(out[:, 7] == 0.0)
    assert np.all(st[:, A + 8] == 1.0) and np.all((code > 0) | (fd == F))
    filled = np.take_along_axis(traj, np.minimum(np.arange(F + 1)[:, None], fd[None, :])[:, :, None], axis=0)
    margins = K.teacher_forced(case, filled)                              # [E, F, 4]
    stepped = np.arange(F)[None, :] < fd[:, None]
    band = K.band4(margins, tol) & stepped
    first = np.where(band.any(axis=1), band.argmax(axis=1), F)
    worst = 0.0
    for e in range(E):
        n = int(fd[e])
        m = margins[e, :n]
        upto = min(n, int(first[e]))
        assert np.all(m[:min(upto, n - 1)] >= 0.0), (e, "the device went on where the twin ends", m[:upto].min(axis=0))
        if first[e] < n:
            continue
        tw_code, tw_frames = K.outcome_from_margins(m[None])
        assert (int(tw_code[0]), int(tw_frames[0])) == (int(code[e]), n) or (tw_code[0] == 0 and code[e] == 0 and n == F), \
            (e, int(tw_code[0]), int(tw_frames[0]), int(code[e]), n, m[-1])
        err = abs(out[e, 6] - m[:, 3].min())
        worst = max(worst, err)
        assert err <= 2 * tol and abs(out[e, 3] - m[:, 1].min()) <= 2 * tol, (e, out[e, 6], m[:, 3].min(), tol)
        if code[e] == 4:
            assert out[e, 6] < 0.0 and out[e, 5] <= -1000.0 + n
    print(f"{name} E={E}: worst outcome[6] error {worst:.2e} (2 tol = {2 * tol:.2e})")
    K.census(case, code, fd, band)


def test_precedence_on_the_device():
    """One step at which several endings hold together (iiwa_like7 with self-collision, floor and sphere): poses in self-contact —
    all of which lie below the floor — give 3; with the obstacle on a capsule, 2; with the target on the end effector, 1; a pose
    below the floor that touches neither itself nor the obstacle, 4."""
    model, twin = K.arm("iiwa_like7")
    rng = np.random.default_rng(5)
    both = C.contact_poses(model, twin, rng, 400)
    both = C.f32(both[(twin.self_clearance(both) < -0.005) & (twin.cell_clearance(both) < -0.005)][:12])
    floor = K.uniform_poses("iiwa_like7", 2048, seed=78)
    floor = floor[(twin.cell_clearance(floor) < -0.005) & (twin.self_clearance(floor) > 0.005)][:4]
    assert len(both) == 12 and len(floor) == 4
    q = np.concatenate([both, floor])
    n = len(q)
    want = np.array([1, 2, 3] * 4 + [4] * 4)
    far_t, far_o = C.away(model)
    target = np.where((want == 1)[:, None], twin.end_effector(q), far_t)
    obstacle = np.where(((want == 2) | ((want == 1) & (np.arange(n) % 6 == 0)))[:, None], twin.world_segments(q)[3][0] + np.zeros((n, 3)), far_o)
    rig = CellRig(model, n, frames=5)
    rig.reset_given(q, target, obstacle)
    rig.load_actions(np.zeros((n, model.A)))
    rig.launch_rollout()
    out = rig.out.cpu().numpy()
    rig.close()
    assert np.array_equal(out[:, 0], want) and np.all(out[:, 1] == 1.0)
    assert np.array_equal(out[:, 5], np.where(want == 1, 250.0, -1000.0)) and np.all(out[:, 6] < -0.004)


# ---- (3) training step -------------------------------------------------------------------------------------------------------------
RANGES = (0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.02)


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("name", ["planar3", "iiwa_like7"])
def test_step_kernel_against_twin(name, ranged):
    """The four instantiations (self-collision pairs: iiwa_like7; scene ranges: `ranged`). E = 100 envs are put on the case's start
    poses and scenes by writing env_state, then stepped 40 times with the case's actions, records on. Every row's reward and done
    are held to the twin's rule at the pose the row was stepped to (float64 from the device's own previous joint values), outside
    the band; a row that ends in workcell contact alone carries -1000 / 1, its env starts a new episode (frame 0, one more episode
    finished, joints back inside the reset range) and its episode record says so."""
    E = 100
    case = K.build_case(name, E)
    model, twin, A, S, tol = case.model, case.twin, case.model.A, case.model.state_size, K.tol_of(case.model)
    lo = np.array([j.lower if j.limited else -np.inf for j in model.joints])
    hi = np.array([j.upper if j.limited else np.inf for j in model.joints])
    init, var = np.array([j.init for j in model.joints]), np.array([j.variation for j in model.joints])
    rig = CellRig(model, E, ranges=RANGES if ranged else None, record_slots=4)
    centre_t, centre_o = np.array([0.3, 0.2, 0.4]), np.array([3.0, 3.0, 3.0])
    rig.reset(centre_t, centre_o)
    st = rig.st.cpu().numpy()
    st[:, :A] = case.q0
    st[:, A:A + 3], st[:, A + 3:A + 6] = case.target, case.obstacle
    rig.st.copy_(torch.from_numpy(st))
    steps = skipped = cell_ends = 0
    for t in range(F):
        prev = rig.st.cpu().numpy()
        rig.load_actions(case.act[:, t])
        rig.launch_step()
        row, now, recs = rig.rows.cpu().numpy(), rig.st.cpu().numpy(), rig.recs.cpu().numpy()
        q = np.clip(prev[:, :A].astype(np.float64) + DT * case.act[:, t], lo, hi)
        m = K.margins4(twin, q, prev[:, A:A + 3].astype(np.float64), prev[:, A + 3:A + 6].astype(np.float64))
        band = K.band4(m, tol)
        reward, done = row[:, rig.off_r], row[:, rig.off_d]
        rec = recs[t % 4]
        for e in range(E):
            steps += 1
            if band[e]:
                skipped += 1
                continue
            ends = m[e] < 0.0
            want = 250.0 if ends[0] else (-1000.0 if ends[1:].any() else None)
            assert done[e] == float(want is not None), (t, e, m[e], reward[e], done[e])
            if want is None:
                assert abs(reward[e] + m[e, 0]) <= tol and now[e, A + 7] == prev[e, A + 7] + 1 and now[e, A + 8] == prev[e, A + 8]
                continue
            assert reward[e] == want, (t, e, m[e], reward[e])
            # the auto-reset: a new episode from the reset range
            assert now[e, A + 7] == 0.0 and now[e, A + 8] == prev[e, A + 8] + 1
            assert np.all(np.abs(now[e, :A] - init) <= var + 1e-6)
            assert rec[e, 3] == 1 and rec[e, 2] == int(prev[e, A + 7]) + 1 and rec[e, 5] == int(now[e, A + 8])
            assert rec[e, 4:5].view(np.float32)[0] == want
            cell_ends += int(ends[3] and not ends[:3].any())
    rig.close()
    print(f"{name} ranged={ranged}: {steps} rows, {skipped} inside the band, {cell_ends} ended by workcell contact alone")
    assert skipped <= K.CAP * steps and cell_ends >= K.FLOOR


# ---- (4) masks ---------------------------------------------------------------------------------------------------------------------
def test_a_cleared_bit_takes_the_pair_out():
    """iiwa_like7 below its floor by 5 cm and more; in the blob the floor bit is cleared on every capsule that comes within 1 cm of
    the floor at any of the poses. No episode ends, and the clearance is that of the pairs left (the twin of the same masks)."""
    model, twin = K.arm("iiwa_like7")
    q = K.uniform_poses("iiwa_like7", 4096, seed=79)
    q = q[(twin.cell_clearance(q) < -0.05) & (twin.self_clearance(q) > 0.01)][:64]
    n = len(q)
    assert n == 64
    floor_bit = 1 << len(model.cell_spheres)
    pairs = twin.cell_clearances(q)                                         # [pairs, n]
    near = {s for k, (s, g) in enumerate(model.cell_pairs) if g == len(model.cell_spheres) and pairs[k].min() < 0.01}
    cut = dataclasses.replace(model, cell_masks=[m & ~floor_bit if s in near else m for s, m in enumerate(model.cell_masks)], _blob=None)
    assert 0 < len(near) and cut.cell_masks != model.cell_masks
    want = KinematicEnvironment(cut, (0, 0, 0), (0, 0, 0)).cell_clearance(q)
    keep = want > 0.01                                                      # (poses that touch the sphere besides are left out)
    assert keep.sum() >= 32
    far_t, far_o = C.away(model)
    outs = []
    for m in (model, cut):
        rig = CellRig(m, n, frames=3)
        rig.reset_given(q, np.tile(far_t, (n, 1)), np.tile(far_o, (n, 1)))
        rc, probe = rig.probe_cell()
        rig.load_actions(np.zeros((n, m.A)))
        rig.launch_rollout()
        outs.append((rc, probe, rig.out.cpu().numpy()))
        rig.close()
    (rc_a, probe_a, out_a), (rc_b, probe_b, out_b) = outs
    assert rc_a == 0 and rc_b == 0
    assert np.all(out_a[:, 0] == 4) and np.all(probe_a < -0.049)
    assert np.all(out_b[keep, 0] == 0) and np.all(out_b[keep, 1] == 1)
    tol = K.tol_of(model)
    assert np.abs(probe_b - want)[keep].max() <= 2 * tol and np.abs(out_b[:, 6] - want)[keep].max() <= 2 * tol


def test_sixteen_geometries_and_bit_15():
    """15 spheres out of reach and the floor as geometry 15: every mask but the base's is 65535, and the floor still ends the
    episode of a pose below it — and of no other."""
    model, twin = K.sixteen()
    assert len(model.cell_spheres) == 15 and model.cell_masks[1:] == [65535] * (len(model.segments) - 1)
    q = K.uniform_poses("iiwa_like7", 1024, seed=80)
    c = twin.cell_clearance(q)
    below, above = q[c < -0.01][:32], q[c > 0.01][:32]
    q = np.concatenate([below, above])
    n = len(q)
    assert len(below) == 32 and len(above) == 32
    far_t, far_o = C.away(model)
    rig = CellRig(model, n, frames=3)
    rig.reset_given(q, np.tile(far_t, (n, 1)), np.tile(far_o, (n, 1)))
    rc, probe = rig.probe_cell()
    rig.load_actions(np.zeros((n, model.A)))
    rig.launch_rollout()
    out = rig.out.cpu().numpy()
    rig.close()
    assert rc == 0 and np.abs(probe - twin.cell_clearance(q)).max() <= 2 * K.tol_of(model)
    assert np.array_equal(out[:, 0], [4.0] * 32 + [0.0] * 32)


# ---- (5) off means off -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planar3", "iiwa_like7"])
def test_without_a_workcell_nothing_changes(name):
    """A model compiled with empty workcell arguments against one compiled without them: rows, observations, env_state and
    outcomes of a fixed-seed training stream and of a rollout are bit-equal, and outcome[6] is 0."""
    kw = {k: v for k, v in K.workcell_of(name).items() if k == "consider_autocollision"}
    models = (K.plain(name), model_of(name, floor_height=None, workcell_planes=[], workcell_spheres=[], cell_ignore=[], **kw))
    case = K.build_case(name, 64)
    results = []
    for model in models:
        rig = CellRig(model, 64, record_slots=4)
        rig.reset((0.3, 0.2, 0.4), (0.2, 0.1, 0.3))
        stream = []
        for t in range(20):
            rig.load_actions(case.act[:, t])
            rig.launch_step(max_frames=7)
            stream += [rig.rows.cpu().numpy().copy(), rig.obs.cpu().numpy().copy(), rig.st.cpu().numpy().copy()]
        stream.append(rig.recs.cpu().numpy().view(np.float32).copy())
        rig.reset_given(case.q0, case.target, case.obstacle)
        for t in range(20):
            rig.load_actions(case.act[:, t])
            rig.launch_rollout()
        out = rig.out.cpu().numpy()
        stream += [out, rig.obs.cpu().numpy(), rig.traj.cpu().numpy()]
        rig.close()
        assert np.all(out[:, 6] == 0.0) and np.all(out[:, 0] != 4)
        results.append(b"".join(bits(a).tobytes() for a in stream))
    assert results[0] == results[1]


# ---- (6) graph capture -------------------------------------------------------------------------------------------------------------
def _graph_of(body):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                                              # (a warm-up launch outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


@pytest.mark.parametrize("ranged", [False, True])
def test_captured_launches_equal_direct_ones(ranged):
    """A captured training step and a captured rollout step, replayed, give the bits of direct launches (iiwa_like7 with its
    workcell, E = 100)."""
    E = 100
    case = K.build_case("iiwa_like7", E)
    runs = []
    for captured in (False, True):
        rig = CellRig(case.model, E, ranges=RANGES if ranged else None, record_slots=4)
        rig.reset((0.3, 0.2, 0.4), (3.0, 3.0, 3.0))
        step = _graph_of(lambda: rig.launch_step(max_frames=9)) if captured else None
        roll = _graph_of(rig.launch_rollout) if captured else None
        for buf in (rig.rows, rig.out, rig.traj, rig.recs):                 # (what the warm-up launches wrote)
            buf.zero_()
        rig.reset((0.3, 0.2, 0.4), (3.0, 3.0, 3.0))
        stream = []
        for t in range(12):
            rig.load_actions(case.act[:, t])
            step.replay() if captured else rig.launch_step(max_frames=9)
            stream += [rig.rows.cpu().numpy().copy(), rig.obs.cpu().numpy().copy(), rig.st.cpu().numpy().copy()]
        stream.append(rig.recs.cpu().numpy().view(np.float32).copy())
        rig.reset_given(case.q0, case.target, case.obstacle)
        for t in range(12):
            rig.load_actions(case.act[:, t])
            roll.replay() if captured else rig.launch_rollout()
        stream += [rig.out.cpu().numpy(), rig.obs.cpu().numpy(), rig.traj.cpu().numpy(), rig.st.cpu().numpy()]
        rig.close()
        runs.append(b"".join(bits(a).tobytes() for a in stream))
    assert runs[0] == runs[1]


# ---- (7) end to end ----------------------------------------------------------------------------------------------------------------
def test_framework_with_a_workcell_end_to_end(scratch_cwd):
    """run_training on iiwa_like7 with floor and sphere at n_envs = 64, scene ranges on; then reach_targets from start poses whose
    wrist hangs 2 to 10 mm above the floor, towards targets below it, with exploration noise: queries end in 'workcell', each
    one's min_cell_clearance is the twin's over its own joint path, and start_cell_clearance the twin's at its start pose."""
    from chain_resume_worker import make_framework
    ee, involved, fixed, init, var = ARM_TABLE["iiwa_like7"]
    reach = model_of("iiwa_like7").reach
    arm = dict(manipulator_file=path("iiwa_like7"), endeffector_index=ee, fixed_joints=fixed, involved_joints=involved,
               target_position=[0.45, -0.3, 0.6], obstacle_position=[0.35, -0.2, 0.45], initial_joint_positions=init,
               initial_positions_variation_range=var, link_radius=0.03, consider_autocollision=True, target_range=[0.15, 0.15, 0.15],
               floor_height=0.0, workcell_spheres=[[0.4 * reach, 0.3 * reach, 0.5 * reach, 0.1 * reach]])
    f = make_framework(arm, checkpoint_frequency=64, save=False)
    scores = f.run_training(64, 50, verbose=False, n_envs=64)
    assert list(scores.keys()) == list(range(1, 65))
    model = f.env.model
    assert model.cell_pairs and model.pack()[10] == 1 and model.pack()[11] == 1
    twin = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0))
    q = K.uniform_poses("iiwa_like7", 8192, seed=81)
    c = twin.cell_clearance(q)
    q = q[(c > 0.002) & (c < 0.010) & (twin.self_clearance(q) > 0.01)][:64]
    N, Fr = len(q), 60
    assert N >= 32
    targets = twin.end_effector(q) - np.array([0.0, 0.0, 0.3])
    out = f.reach_targets(targets, obstacles=[3.0, 3.0, 3.0], initial_joint_positions=q, frames=Fr, noise_scale=1.0)
    tol = K.tol_of(model)
    assert set(out.outcome) <= {"reached", "obstacle", "self", "workcell", "frames"} and np.sum(out.outcome == "workcell") >= 1
    assert out.min_cell_clearance.dtype == np.float32 and out.start_cell_clearance.shape == (N,)
    assert np.abs(out.start_cell_clearance - twin.cell_clearance(q.astype(np.float32).astype(np.float64))).max() <= 2 * tol
    for i in range(N):
        own = twin.cell_clearance(out.joint_positions[i, 1:out.frames[i] + 1].astype(np.float64))
        assert abs(out.min_cell_clearance[i] - own.min()) <= 2 * tol, (i, out.min_cell_clearance[i], own.min())
        if out.outcome[i] == "workcell":
            assert out.min_cell_clearance[i] < 0.0 and own[-1] < 2 * tol and np.all(own[:-1] > -2 * tol)
    # without a workcell the two fields are +inf
    plain = dict(arm)
    for k in ("floor_height", "workcell_spheres"):
        plain.pop(k)
    g = make_framework(plain, checkpoint_frequency=64, save=False)
    one = g.reach_targets(targets[:4], obstacles=[3.0, 3.0, 3.0], initial_joint_positions=q[:4], frames=5)
    assert np.all(np.isposinf(one.min_cell_clearance)) and np.all(np.isposinf(one.start_cell_clearance))
    assert "workcell" not in set(one.outcome)
