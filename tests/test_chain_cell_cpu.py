"""CPU (`-m "not gpu"`): the workcell of the kinematic arm environment — floor, walls and fixed spheres — in the chain model
compiler (environment/urdf_chain.py), the float64 twin (environment/kinematic.py), the packed blob and the library's host-side
check of it, the framework's refusals, and a rehearsal of the GPU cases with the twin alone."""
import dataclasses
import logging

import numpy as np
import pytest

import chain_cell_common as K
import chain_rollout_common as C
from test_chain_env_cpu import ARMS as ARM_TABLE
from test_chain_env_cpu import model_of, path, random_q

from robotic_manipulator_rloa_amd.environment import urdf_chain as UC
from robotic_manipulator_rloa_amd.environment.kinematic import OUTCOMES, KinematicEnvironment, cell_box_gaps
from robotic_manipulator_rloa_amd.utils.exceptions import InvalidManipulatorFile

ERR_CELL, ERR_PAIRS = -21, -19


def _lib():
    from robotic_manipulator_rloa_amd import _lib
    return _lib.load()


def _check(blob):
    blob = np.ascontiguousarray(blob, np.float32)
    return _lib().naf_chain_env_model_check(blob.ctypes.data, int(blob.size))


# ---- the blob ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.ARMS)
def test_blob_round_trip(name):
    """Header [10] = G, [11] = H; behind the pair table G x 4 sphere floats, H x 4 half-space floats, one mask per segment; the
    library accepts it, and the digest tells it from the arm without a workcell."""
    model, _ = K.arm(name)
    base = K.plain(name)
    blob, b0 = model.pack(), base.pack()
    G, H, n_seg = len(model.cell_spheres), len(model.cell_planes), len(model.segments)
    assert blob.dtype == np.float32 and (blob[10], blob[11]) == (G, H) and np.all(blob[12:16] == 0)
    assert blob[0] == UC.BLOB_VERSION == 1 and blob[8] == blob.size == b0.size + 4 * (G + H) + n_seg
    assert np.array_equal(blob[16:b0.size], b0[16:]) and np.array_equal(blob[:8], b0[:8]) and blob[9] == b0[9]
    tail = blob[b0.size:]
    assert np.array_equal(tail[:4 * G].reshape(G, 4), np.float32(model.cell_spheres).reshape(G, 4))
    assert np.array_equal(tail[4 * G:4 * (G + H)].reshape(H, 4), np.float32(model.cell_planes).reshape(H, 4))
    assert np.array_equal(tail[4 * (G + H):], np.float32(model.cell_masks)) and len(model.cell_masks) == n_seg
    assert _check(blob) == 0 and _check(b0) == 0
    assert model.digest() != base.digest()
    assert _lib().naf_hip_abi_version() == 40


@pytest.mark.parametrize("name", K.ARMS)
def test_no_workcell_is_byte_equal(name):
    """G = H = 0: pack() is byte for byte the blob of a model compiled without the arguments."""
    kw = {k: v for k, v in K.workcell_of(name).items() if k == "consider_autocollision"}
    empty = model_of(name, floor_height=None, workcell_planes=[], workcell_spheres=None, cell_ignore=[], **kw)
    assert empty.pack().tobytes() == K.plain(name).pack().tobytes() and empty.digest() == K.plain(name).digest()
    assert empty.cell_masks == [] and empty.cell_pairs == []
    twin = KinematicEnvironment(empty, (0, 0, 0), (0, 0, 0))
    assert np.all(np.isposinf(twin.cell_clearance(K.uniform_poses(name)[:8]))) and twin.cell_clearance(np.zeros(empty.A)) == np.inf


def test_model_check_names_every_malformed_field():
    model, _ = K.arm("iiwa_like7")
    good = model.pack()
    n0 = K.plain("iiwa_like7").pack().size
    G, H, n_seg = 1, 1, len(model.segments)
    assert _check(good) == 0

    def bad(**edits):
        b = good.copy()
        for k, v in edits.items():
            b[int(k[1:])] = v
        return _check(b)
    # counts out of range
    assert bad(_10=17) == ERR_CELL and bad(_10=-1) == ERR_CELL and bad(_10=0.5) == ERR_CELL
    assert bad(_10=16, _11=1) == ERR_CELL and bad(_11=17) == ERR_CELL
    # a count that does not match the blob's size; a blob cut short or padded
    assert bad(_10=2) == ERR_CELL and bad(_11=0) == ERR_CELL
    for size in (good.size - 1, good.size + 1, good.size - n_seg):
        b = np.resize(good, size)
        b[size - 1] = 0
        b[8] = size
        assert _check(b) == ERR_CELL, size
    # a negative radius, a normal that is not a unit vector
    assert bad(**{f"_{n0 + 3}": -0.01}) == ERR_CELL
    assert bad(**{f"_{n0 + 4 + 2}": 1.01}) == ERR_CELL and bad(**{f"_{n0 + 4 + 2}": 0.0}) == ERR_CELL
    # a mask that is not an integer in range (G + H = 2: 0 .. 3)
    first = n0 + 4 * (G + H)
    assert bad(**{f"_{first}": 4}) == ERR_CELL and bad(**{f"_{first + 3}": 1.5}) == ERR_CELL and bad(**{f"_{first + n_seg - 1}": -1}) == ERR_CELL
    assert bad(**{f"_{first}": 0}) == 0 and bad(**{f"_{first}": 3}) == 0
    # verdicts of before: a non-finite value is still NAF_CHAIN_ERR_VALUE, an old blob with a wrong pair table still ERR_PAIRS
    assert bad(**{f"_{n0 + 1}": np.inf}) == -14
    old = K.plain("iiwa_like7").pack()
    old[9] += 1
    assert _check(old) == ERR_PAIRS
    # 16 geometries: masks up to 65535 are exact
    m16, _ = K.sixteen()
    b16 = m16.pack()
    assert (b16[10], b16[11]) == (15, 1) and _check(b16) == 0 and max(m16.cell_masks) == 65535 and b16[-1] == 65535.0


# ---- the compiler ----------------------------------------------------------------------------------------------------------------
def test_pruning_on_the_three_arms():
    """The base capsule stands on the floor at every pose and is dropped, by name; nothing else is. A floor under planar3, which
    lies in z = 0, touches every capsule at every pose and is refused by name."""
    iiwa, _ = K.arm("iiwa_like7")
    long12, _ = K.arm("long12")
    planar, _ = K.arm("planar3")
    assert iiwa.cell_pairs_dropped == [(iiwa.segments[0].link_name, 1)] and long12.cell_pairs_dropped == [(long12.segments[0].link_name, 0)]
    assert iiwa.cell_masks == [1] + [3] * (len(iiwa.segments) - 1)            # sphere = bit 0, floor = bit 1
    assert long12.cell_masks == [0] + [1] * (len(long12.segments) - 1)
    assert planar.cell_pairs_dropped == [] and planar.cell_masks == [3] * len(planar.segments)
    assert iiwa.cell_planes == [(0.0, 0.0, 1.0, 0.0)] and len(iiwa.cell_pairs) == sum(bin(m).count("1") for m in iiwa.cell_masks)
    with pytest.raises(InvalidManipulatorFile, match=r"workcell plane 0 \(normal 0 0 1, offset 0\) is left with no capsule"):
        model_of("planar3", floor_height=0.0)
    # cell_ignore drops more, by link name or index; a geometry it empties is refused
    link = iiwa.segments[-1].link_name
    fewer = model_of("iiwa_like7", **dict(K.workcell_of("iiwa_like7"), cell_ignore=[(link, 1), (iiwa.segments[2].link, 0)]))
    assert fewer.cell_masks[-1] == 1 and fewer.cell_masks[2] == 2 and fewer.cell_pairs_dropped == iiwa.cell_pairs_dropped
    with pytest.raises(InvalidManipulatorFile, match="cell_ignore names the link 'nolink'"):
        model_of("long12", floor_height=0.0, cell_ignore=[("nolink", 0)])
    with pytest.raises(InvalidManipulatorFile, match="cell_ignore names workcell geometry 1"):
        model_of("long12", floor_height=0.0, cell_ignore=[(long12.segments[1].link_name, 1)])
    with pytest.raises(InvalidManipulatorFile, match="left with no capsule"):
        model_of("long12", floor_height=0.0, cell_ignore=[(s.link_name, 0) for s in long12.segments])
    with pytest.raises(InvalidManipulatorFile, match="not a unit vector"):
        model_of("long12", workcell_planes=[(0.0, 0.0, 2.0, 0.0)])
    with pytest.raises(InvalidManipulatorFile, match="negative radius"):
        model_of("long12", workcell_spheres=[(1.0, 1.0, 1.0, -0.1)])
    with pytest.raises(InvalidManipulatorFile, match="at most 16"):
        model_of("long12", workcell_spheres=[(5.0, 5.0, 5.0 + k, 0.1) for k in range(17)])


# ---- the twin --------------------------------------------------------------------------------------------------------------------
def test_cell_clearance_is_the_rule_stated_once():
    """cell_clearance against the rule written out per pose with plain loops; batched like clearance."""
    for name in K.ARMS:
        model, twin = K.arm(name)
        q = K.uniform_poses(name)[:40]
        got = twin.cell_clearance(q)
        assert got.shape == (40,)
        G = len(model.cell_spheres)
        for i in range(40):
            best = np.inf
            for s, (a, b, rho) in enumerate(twin.world_segments(q[i])):
                for g in range(G + len(model.cell_planes)):
                    if not model.cell_masks[s] >> g & 1:
                        continue
                    if g < G:
                        c = np.array(model.cell_spheres[g])
                        t = np.clip(np.dot(c[:3] - a, b - a) / max(np.dot(b - a, b - a), 1e-300), 0.0, 1.0)
                        best = min(best, np.linalg.norm(a + t * (b - a) - c[:3]) - rho - c[3])
                    else:
                        n = np.array(model.cell_planes[g - G])
                        best = min(best, min(np.dot(n[:3], a), np.dot(n[:3], b)) - n[3] - rho)
            assert abs(got[i] - best) <= 1e-12 and twin.cell_clearance(q[i]) == got[i]
        assert twin.cell_clearance(q.reshape(5, 8, -1)).shape == (5, 8)


@pytest.mark.parametrize("name", K.ARMS)
def test_trace_equals_step_with_a_workcell(name):
    """trace's code, frames, score, distances and clearances, the workcell's among them, against a loop over step()."""
    case = K.build_case(name, 64)
    model, twin = case.model, case.twin
    T = twin.trace(case.q0, case.act, case.target, case.obstacle, K.FRAMES)
    assert T.cell_margins.shape == (64, K.FRAMES) and T.margins.shape == (64, K.FRAMES, 3) and OUTCOMES[4] == "workcell"
    for i in range(64):
        env = KinematicEnvironment(model, case.target[i], case.obstacle[i], K.ORAD)
        env.q = case.q0[i].copy()
        score, least, n, reward, done = 0.0, np.inf, 0, 0.0, 0
        for t in range(K.FRAMES):
            _, reward, done = env.step(case.act[i, t])
            n, score, least = n + 1, score + reward, min(least, env.last_cell_clearance)
            assert T.cell_margins[i, t] == env.last_cell_clearance
            if done:
                break
        assert T.frames[i] == n and T.score[i] == score and T.min_cell_clearance[i] == least
        want = 0 if not done else (1 if reward == 250 else (2 if env.last_clearance < K.ORAD else (3 if env.last_self_clearance < 0 else 4)))
        assert T.code[i] == want and np.all(np.isnan(T.cell_margins[i, n:]))
        if want == 4:
            assert reward == -1000 and env.last_cell_clearance < 0.0
    assert set(np.unique(T.code)) == set(case.outcomes)


def test_precedence_in_the_twin():
    """A pose below the floor that also touches the obstacle gives 'obstacle'; with the target on its end effector, 'reached'."""
    model, twin = K.arm("long12")
    q = K.uniform_poses("long12")
    q = q[twin.cell_clearance(q) < -0.01][:4]
    on_arm = twin.world_segments(q)[3][0]
    far_t, far_o = C.away(model)
    zero = np.zeros((4, 1, model.A))
    assert np.all(twin.trace(q, zero, far_t, far_o, 1).code == 4)
    assert np.all(twin.trace(q, zero, far_t, on_arm, 1).code == 2)
    assert np.all(twin.trace(q, zero, twin.end_effector(q), on_arm, 1).code == 1)
    assert np.all(twin.trace(q, zero, far_t, far_o, 1).score == -1000.0)


# ---- the host --------------------------------------------------------------------------------------------------------------------
def _framework():
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    return ManipulatorFramework()


def _iiwa(**over):
    ee, involved, fixed, init, var = ARM_TABLE["iiwa_like7"]
    kw = dict(manipulator_file=path("iiwa_like7"), endeffector_index=ee, fixed_joints=fixed, involved_joints=involved,
              target_position=[0.45, 0.3, 0.6], obstacle_position=[0.35, 0.2, 0.45], initial_joint_positions=init,
              initial_positions_variation_range=var, link_radius=0.03, consider_autocollision=True, floor_height=0.0)
    kw.update(over)
    return kw


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_framework_passes_the_workcell_through_and_logs_the_share():
    from robotic_manipulator_rloa_amd.utils.logger import get_global_logger
    f = _framework()
    log, lines = get_global_logger(), _Lines()
    log.addHandler(lines)
    try:
        f.initialize_kinematic_environment(**_iiwa(workcell_spheres=[[0.2, -0.5, 0.5, 0.1]], workcell_planes=[[1.0, 0.0, 0.0, -0.6]],
                                                   cell_ignore=[("link_7", 0)]))
    finally:
        log.removeHandler(lines)
    m = f.env.model
    assert m.cell_spheres == [(0.2, -0.5, 0.5, 0.1)] and m.cell_planes == [(0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, -0.6)]
    assert m.cell_pairs_dropped == [("link_0", 1)] and m.cell_masks[-1] & 1 == 0
    assert any("% of 1024 sampled episode starts are in workcell contact" in line for line in lines.lines)
    copy = f._env_factory()
    assert copy.model.digest() == m.digest() and copy.model.digest() != model_of("iiwa_like7", consider_autocollision=True).digest()
    state, reward, done = f.env.step(np.zeros(7))
    assert state.shape == (23,) and done == 0                      # S = 2A + 9: the workcell has no slot


def test_framework_refusals():
    f = _framework()
    init = ARM_TABLE["iiwa_like7"][3]
    twin = KinematicEnvironment(model_of("iiwa_like7"), (0, 0, 0), (0, 0, 0))
    tip = twin.end_effector(np.array(init))
    with pytest.raises(ValueError, match=r"at the initial joint positions the link '.*' is in contact with workcell sphere 0 .* cell_ignore="):
        f.initialize_kinematic_environment(**_iiwa(workcell_spheres=[[float(tip[0]), float(tip[1]), float(tip[2]), 0.05]]))
    with pytest.raises(ValueError, match=r"the target lies within 0\.0400 m of workcell plane 1 \(normal 0 -1 0, offset -0\.34\)"):
        f.initialize_kinematic_environment(**_iiwa(workcell_planes=[[0.0, -1.0, 0.0, -0.34]]))
    with pytest.raises(ValueError, match=r"the target box .* comes within 0\.0600 m of workcell plane 1"):
        f.initialize_kinematic_environment(**_iiwa(workcell_planes=[[0.0, -1.0, 0.0, -0.46]], target_range=[0.1, 0.1, 0.1]))
    # 0.06 is enough for a fixed target (0.05), not for a box with scene_margin 0.02 (0.07)
    f.initialize_kinematic_environment(**_iiwa(workcell_planes=[[0.0, -1.0, 0.0, -0.36]]))
    with pytest.raises(ValueError, match=r"workcell sphere 0"):
        f.initialize_kinematic_environment(**_iiwa(workcell_spheres=[[0.45, 0.3, 0.8, 0.1]], target_range=[0.0, 0.0, 0.06]))
    # most sampled starts in contact: the nominal start pose lies in the plane y = 0 (capsule radius 0.06, the base's), between
    # two walls 1 mm clear of it; the first joint's +-0.1 rad swings the arm into one of them
    assert max(abs(p[1]) + r for a, b, r in twin.world_segments(np.array(init)) for p in (a, b)) < 0.0601
    with pytest.raises(ValueError, match=r"of 1024 sampled episode starts .* are in workcell contact"):
        f.initialize_kinematic_environment(**_iiwa(workcell_planes=[[0.0, -1.0, 0.0, -0.061], [0.0, 1.0, 0.0, -0.061]],
                                                   target_position=[0.45, 0.0, 0.6]))
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    with pytest.raises(InvalidEnvironmentParameter, match="Floor height"):
        f.initialize_kinematic_environment(**_iiwa(floor_height="low"))
    with pytest.raises(InvalidEnvironmentParameter, match="Workcell spheres"):
        f.initialize_kinematic_environment(**_iiwa(workcell_spheres=[[0.0, 0.0, 1.0]]))
    with pytest.raises(InvalidManipulatorFile, match="left with no capsule"):
        f.initialize_kinematic_environment(**_iiwa(floor_height=2.0))


def test_box_against_geometry_is_brute_force():
    """cell_box_gaps against dense sampling of the box (its corners and faces included): never above the sampled minimum, and
    within the sampling's resolution of it."""
    model, _ = K.sixteen()
    model = dataclasses.replace(model, cell_planes=[(0.0, 0.0, 1.0, 0.0), (0.6, -0.8, 0.0, -0.2), (-0.48, 0.6, 0.64, -0.3)],
                                cell_spheres=[(0.3, 0.2, 0.5, 0.1), (0.9, 0.9, 0.9, 0.3)], _blob=None)
    rng = np.random.default_rng(3)
    for _ in range(20):
        centre, half = rng.uniform(-0.5, 1.0, 3), rng.uniform(0.0, 0.4, 3) * (rng.random(3) > 0.2)
        grid = np.stack(np.meshgrid(*[np.linspace(c - h, c + h, 21) for c, h in zip(centre, half)], indexing="ij"), axis=-1).reshape(-1, 3)
        sampled = [np.min(np.linalg.norm(grid - np.array(c[:3]), axis=1)) - c[3] for c in model.cell_spheres]
        sampled += [np.min(grid @ np.array(n[:3])) - n[3] for n in model.cell_planes]
        got = cell_box_gaps(model, centre, half)
        step = np.linalg.norm(half) / 10.0
        assert np.all(got <= np.array(sampled) + 1e-12) and np.all(got >= np.array(sampled) - step - 1e-12)
        assert np.allclose(got[2:], sampled[2:], atol=1e-12)              # a half-space's minimum is at a corner: sampled exactly
    assert np.allclose(cell_box_gaps(model, (0.3, 0.2, 0.5), (0.0, 0.0, 0.0))[:1], [-0.1])


# ---- rehearsal of the GPU cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", K.SIZES)
@pytest.mark.parametrize("name", K.ARMS)
def test_rehearsal_of_the_rollout_cases(name, E):
    """The twin alone on the cases of tests/test_chain_cell_gpu.py: every env ends as it was built to, at least 8 envs in each
    outcome the arm can have (E >= 64), and at most 1 % of the (env, step) pairs inside the band."""
    case = K.build_case(name, E)
    T = case.twin.trace(case.q0, case.act, case.target, case.obstacle, K.FRAMES)
    m = np.concatenate([T.margins, T.cell_margins[..., None]], axis=-1)
    stepped = np.arange(K.FRAMES)[None, :] < T.frames[:, None]
    band = K.band4(m, K.tol_of(case.model)) & stepped
    counts, skipped, total = K.census(case, T.code, T.frames, band)
    assert np.array_equal(T.code, case.want)
    assert np.all(T.min_cell_clearance[T.code == 4] < 0.0) and np.all(T.min_cell_clearance[T.code != 4] >= 0.0)


@pytest.mark.parametrize("name", K.ARMS)
def test_rehearsal_of_the_probe_poses(name):
    """Of the probe's uniform poses at most 1 % lie within 2 tol of contact, and both signs occur."""
    model, twin = K.arm(name)
    c = twin.cell_clearance(K.uniform_poses(name))
    inside = np.abs(c) <= 2 * K.tol_of(model)
    print(f"{name}: {np.mean(c < 0):.3f} of {len(c)} poses in workcell contact, {int(inside.sum())} inside the band")
    assert inside.sum() <= 0.01 * len(c) and np.sum(c < 0) >= 8 and np.sum(c > 0) >= 8
