"""CPU (`-m "not gpu"`): the URDF -> chain model compiler (environment/urdf_chain.py), its float64 host twin
(environment/kinematic.py), the packed blob and the library's host-side check of it, and the framework plumbing."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN

from robotic_manipulator_rloa_amd.environment import urdf_chain as UC
from robotic_manipulator_rloa_amd.environment.kinematic import KinematicEnvironment, build_kinematic, segment_point_distance2
from robotic_manipulator_rloa_amd.utils.exceptions import InvalidManipulatorFile

URDF = os.path.join(GOLDEN, "urdf")
# name -> (endeffector_index, involved_joints, fixed_joints, initial_joint_positions, variation)
ARMS = {
    "planar3": (2, [0, 1, 2], [], [0.3, -0.4, 0.5], [0.1, 0.1, 0.1]),
    "iiwa_like7": (6, [0, 1, 2, 3, 4, 5, 6], [7], [0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0], [0.1, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2]),
    "arm_with_gripper": (7, [1, 2, 3, 4, 5, 6], [0, 7, 8, 9], [0., 0.4, 0., -1.0, 0., 0.5, 0.], [0, 0, 0, 0.3, 0.5, 0.5, 0.5]),
    "standin8": (7, list(range(8)), [], [0.9, 0.45, 0, 0, 0, 0, 0, 0], [0.1] * 8),
    "long12": (11, list(range(12)), [], [0.1 * ((k % 5) - 2) for k in range(12)], [0.05] * 12),
    "long32": (31, list(range(32)), [], [0.1 * ((k % 5) - 2) for k in range(32)], [0.05] * 32),
    "slider4": (3, [0, 1, 2, 3], [], [0.2, 0.1, 0.3, 0.1], [0.1] * 4),      # chain_ik_common.slider's: joints 1 and 3 prismatic
}


def path(name):
    return os.path.join(URDF, name + ".urdf")


def model_of(name, link_radius=0.03, **over):
    ee, involved, fixed, init, var = ARMS[name]
    kw = dict(endeffector_index=ee, involved_joints=involved, fixed_joints=fixed, initial_joint_positions=init,
              initial_positions_variation_range=var, link_radius=link_radius)
    kw.update(over)
    return UC.compile_chain(UC.load_urdf(path(name)), **kw)


def env_of(name, target=(0.3, 0.2, 0.4), obstacle=(5.0, 5.0, 5.0), **over):
    return KinematicEnvironment(model_of(name, **over), target, obstacle)


def random_q(model, rng):
    return np.array([rng.uniform(j.lower, j.upper) if j.limited else rng.uniform(-np.pi, np.pi) for j in model.joints])


# ---- 1. known answers ----------------------------------------------------------------------------------------------------
def test_planar3_end_effector_is_the_textbook_sum():
    """Three z joints, links 0.3 / 0.25 / 0.15 along x: ee = sum_i l_i (cos(q_0 + .. + q_i), sin(q_0 + .. + q_i), 0)."""
    env = env_of("planar3")
    grid = np.linspace(-3.0, 3.0, 7)
    for q0 in grid:
        for q1 in grid:
            for q2 in grid:
                c = np.cumsum([q0, q1, q2])
                want = np.array([np.sum(np.array([0.3, 0.25, 0.15]) * np.cos(c)), np.sum(np.array([0.3, 0.25, 0.15]) * np.sin(c)), 0.0])
                np.testing.assert_allclose(env.end_effector(np.array([q0, q1, q2])), want, atol=1e-14)


def test_iiwa_like7_hand_computed_poses():
    """At q = 0 the arm stands straight up: the last joint's origin is at z = 0.1575 + 0.2025 + 0.2045 + 0.2155 + 0.1845 + 0.2155
    + 0.081 = 1.261 and the tip (inertial origin 0.02 further along the last link's z) at 1.281.
    Joint 1 (the second) sits at z = 0.1575 + 0.2025 = 0.36; its rpy (pi/2, 0, pi) turns its z axis onto world +y. A quarter turn
    about +y carries +z onto +x, so the 1.261 - 0.36 = 0.901 above it lie along +x: last joint origin (0.901, 0, 0.36).
    Joint 3 (the fourth) sits at z = 0.36 + 0.2045 + 0.2155 = 0.78 with its z axis on world -y (the alternation flips it). A quarter
    turn about -y carries +z onto -x: the 1.261 - 0.78 = 0.481 above it lie along -x: (-0.481, 0, 0.78).
    Both: joint 3 has moved to (0.42, 0, 0.36) (0.2045 + 0.2155 = 0.42 along +x) and its axis, parallel to y, is unchanged; the
    quarter turn about -y carries the +x direction of the upper arm onto +z: (0.42, 0, 0.36 + 0.481) = (0.42, 0, 0.841)."""
    env = env_of("iiwa_like7")
    last = lambda q: env.frames(np.array(q, float))[7][1]      # noqa: E731
    np.testing.assert_allclose(last([0] * 7), [0, 0, 1.261], atol=1e-12)
    np.testing.assert_allclose(env.end_effector(np.zeros(7)), [0, 0, 1.281], atol=1e-12)
    h = np.pi / 2
    np.testing.assert_allclose(last([0, h, 0, 0, 0, 0, 0]), [0.901, 0, 0.36], atol=1e-12)
    np.testing.assert_allclose(last([0, 0, 0, h, 0, 0, 0]), [-0.481, 0, 0.78], atol=1e-12)
    np.testing.assert_allclose(last([0, h, 0, h, 0, 0, 0]), [0.42, 0, 0.841], atol=1e-12)
    np.testing.assert_allclose(env.end_effector(np.array([0, h, 0, h, 0, 0, 0])), [0.42, 0, 0.861], atol=1e-12)


def test_standin8_is_the_stand_ins_chain():
    """environment.synthetic.forward_kinematics is a separately written statement of the same eight-joint chain."""
    from robotic_manipulator_rloa_amd.environment import synthetic
    env = env_of("standin8")
    rng = np.random.default_rng(1)
    for _ in range(1000):
        q = rng.uniform(-np.pi, np.pi, 8)
        ee, _ = synthetic._fk_fast(q.tolist(), (9.0, 9.0, 9.0))
        np.testing.assert_allclose(env.end_effector(q), ee, atol=1e-6)
    ee32, _ = synthetic.forward_kinematics(q.astype(np.float32), np.array([9, 9, 9], np.float32))
    np.testing.assert_allclose(env.end_effector(q), ee32, atol=2e-6)


# ---- 2. an independent forward kinematics ---------------------------------------------------------------------------------
def independent_fk(name, q_by_joint_index):
    """4 x 4 homogeneous matrices over the URDF tree, scipy rotations, read from the XML here: {link: T_world_link}, and under
    ("joint", k) the frame of joint k's origin."""
    import xml.etree.ElementTree as ET
    from scipy.spatial.transform import Rotation
    root = ET.parse(path(name)).getroot()
    T = {}
    joints = root.findall("joint")
    children = {j.find("child").get("link") for j in joints}
    for l in root.findall("link"):
        if l.get("name") not in children:
            T[l.get("name")] = np.eye(4)
    pending = list(enumerate(joints))
    while pending:
        k, j = pending.pop(0)
        parent = j.find("parent").get("link")
        if parent not in T:
            pending.append((k, j))
            continue
        o = j.find("origin")
        xyz = [float(v) for v in o.get("xyz").split()]
        rpy = [float(v) for v in o.get("rpy").split()]
        M = np.eye(4)
        M[:3, :3] = Rotation.from_euler("xyz", rpy).as_matrix()      # extrinsic x, y, z = Rz(yaw) Ry(pitch) Rx(roll)
        M[:3, 3] = xyz
        Q = np.eye(4)
        q = q_by_joint_index.get(k, 0.0)
        if j.get("type") in ("revolute", "continuous"):
            ax = np.array([float(v) for v in j.find("axis").get("xyz").split()])
            Q[:3, :3] = Rotation.from_rotvec(ax / np.linalg.norm(ax) * q).as_matrix()
        elif j.get("type") == "prismatic":
            ax = np.array([float(v) for v in j.find("axis").get("xyz").split()])
            Q[:3, 3] = ax / np.linalg.norm(ax) * q
        T[("joint", k)] = T[parent] @ M                           # the joint's origin, before its own motion
        T[j.find("child").get("link")] = T[parent] @ M @ Q
    return T, joints, root


@pytest.mark.parametrize("name", list(ARMS))
def test_twin_agrees_with_an_independent_fk(name):
    ee_index, involved, fixed, init, _ = ARMS[name]
    env = env_of(name)
    rng = np.random.default_rng(2)
    import xml.etree.ElementTree as ET  # noqa: F401
    for _ in range(1000):
        q = random_q(env.model, rng)
        T, joints, root = independent_fk(name, {k: q[m] for m, k in enumerate(involved)})
        link = joints[ee_index].find("child").get("link")
        el = [l for l in root.findall("link") if l.get("name") == link][0]
        local = np.zeros(3)
        if el.find("inertial") is not None:
            local = np.array([float(v) for v in el.find("inertial/origin").get("xyz").split()])
        want = (T[link] @ np.append(local, 1.0))[:3]
        assert np.abs(env.end_effector(q) - want).max() <= 1e-12 * env.model.reach
    # every capsule's ends are joint origins (or the tip) of that independent tree: a link's capsule ends where its child joint
    # sits on it, which a prismatic joint's travel (slider4) carries the child link's own origin away from
    ends = [T[("joint", k)][:3, 3] for k in range(len(joints))] + [T[j.find("child").get("link")][:3, 3] for j in joints] + \
        [want, np.zeros(3)]
    for a, b, _ in env.world_segments(q):
        for p in (a, b):
            assert min(np.abs(p - e).max() for e in ends) <= 1e-12 * env.model.reach


# ---- 3. index rules -------------------------------------------------------------------------------------------------------
def test_index_rules_on_the_arm_with_a_gripper():
    """The xArm quirk: a fixed world joint is joint 0, so involved_joints = [1..6]."""
    ee_index, involved, fixed, init, var = ARMS["arm_with_gripper"]
    env = env_of("arm_with_gripper")
    m = env.model
    assert [j.index for j in m.joints] == involved and m.A == 6
    # reset applies entry k to joint INDEX k (environment.py:284-293)
    assert [j.init for j in m.joints] == [init[k] for k in involved]
    assert [j.variation for j in m.joints] == [var[k] for k in involved]
    s0 = env.reset(False)
    for k, j in enumerate(m.joints):
        assert abs(env.q[k] - j.init) <= j.variation
    # slot k reports joint index k: slot 0 is the fixed world joint (always 0), slots 1..5 the first five driven joints
    assert s0[0] == 0.0 and s0[6] == 0.0
    np.testing.assert_array_equal(s0[1:6], env.q[:5])
    # action k moves joint involved[k]
    for k in range(6):
        env.reset(False)
        before = env.q.copy()
        a = np.zeros(6)
        a[k] = 0.5
        s, _, _ = env.step(a)
        moved = np.nonzero(env.q != before)[0].tolist()
        assert moved == [k]
        assert s[0] == 0.0 and s[6] == 0.0
        if k < 5:
            assert s[6 + k + 1] == 0.5 and s[k + 1] == env.q[k]
        else:                                       # joint index 6 has no slot (environment.py:442-444 reads indices 0 .. A-1)
            np.testing.assert_array_equal(s[6:12], 0.0)
    # the held fingers stay at 0 and their segments ride on the last driven joint's frame
    assert m.ee_frame == 6
    assert sorted(s.frame for s in m.segments).count(6) == 4      # link6 -> gripper, gripper -> two fingers, gripper -> tip
    T, joints, _ = independent_fk("arm_with_gripper", {k: env.q[i] for i, k in enumerate(involved)})
    finger = T["finger_left"][:3, 3]
    assert min(np.abs(b - finger).max() for _, b, _ in env.world_segments()) < 1e-12
    # a parked joint (movable, neither driven nor held) keeps its initial value: drive only joints 1..5, leave 6 free
    m5 = model_of("arm_with_gripper", involved_joints=[1, 2, 3, 4, 5], fixed_joints=[0, 7, 8, 9],
                  initial_joint_positions=[0, 0, 0, 0, 0, 0, 0.7])
    e5 = KinematicEnvironment(m5, (0, 0, 0), (5, 5, 5))
    T, _, _ = independent_fk("arm_with_gripper", {6: 0.7})
    np.testing.assert_allclose(e5.end_effector(np.zeros(5)), (T["gripper_base"] @ [0, 0, 0.03, 1])[:3], atol=1e-12)


# ---- 4. reward / terminal rule, limits, protocol ---------------------------------------------------------------------------
def _oracle_says(env):
    """(reward, done) by oracle/env_oracle.py — the rule as fixture G9 pins it on the reference — of what the last step exposed"""
    from oracle import env_oracle
    return env_oracle.rule(env.last_distance, [env.last_clearance - env.obstacle_radius, env.last_cell_clearance],
                           [env.last_self_clearance], bool(env.model.self_pairs))


def test_reward_and_terminal_rule_at_the_thresholds():
    env = env_of("iiwa_like7")
    q = np.array([0.2, 0.5, -0.3, -1.0, 0.4, 0.7, 0.1])
    ee = env.end_effector(q)
    d = np.array([0.0, 0.6, 0.8])
    for dist, reached in ((0.05 - 1e-9, True), (0.05 + 1e-9, False)):
        env.q = q.copy()
        env.target_pos = ee + dist * d
        s, r, done = env.step(np.zeros(7))
        assert (r == 250 and done == 1) if reached else (done == 0 and abs(r + 1e-9) < 1e-12)
        assert (r, done) == _oracle_says(env)
    env.target_pos = ee + 0.3 * d
    env.q = q.copy()
    s, r, done = env.step(np.zeros(7))
    assert done == 0 and abs(r + 0.25) < 1e-12 and abs(env.last_distance - 0.3) < 1e-12
    # contact: the obstacle centre at radius + obstacle radius -/+ 1e-9 from the middle of a capsule, perpendicular to it
    a, b, rad = [s for s in env.world_segments(q) if np.linalg.norm(s[1] - s[0]) > 0.1][2]
    u = (b - a) / np.linalg.norm(b - a)
    n = np.cross(u, [0.3, 0.5, 0.8])
    n /= np.linalg.norm(n)
    for off, hit in ((-1e-9, True), (1e-9, False)):
        env.q = q.copy()
        env.obstacle_pos = 0.5 * (a + b) + (rad + env.obstacle_radius + off) * n
        # (other capsules must not be nearer: checked through the clearance the twin reports)
        s, r, done = env.step(np.zeros(7))
        assert abs(env.last_clearance - (env.obstacle_radius + off)) < 1e-12
        assert (r == -1000 and done == 1) if hit else (done == 0 and r < 0)
        assert (r, done) == _oracle_says(env)
    # reaching wins over contact (environment.py:345-371 tests the target first)
    env.q = q.copy()
    env.target_pos = ee.copy()
    env.obstacle_pos = ee.copy()
    assert env.step(np.zeros(7))[1:] == (250, 1) == _oracle_says(env)
    assert segment_point_distance2(np.zeros(3), np.array([1.0, 0, 0]), np.array([2.0, 1.0, 0])) == 2.0     # clamped to the end


def test_limit_clamp_zeroes_the_reported_velocity():
    env = env_of("iiwa_like7")
    env.reset(False)
    hi = env.model.joints[1].upper
    env.q[1] = hi - 1e-4
    s, _, _ = env.step(np.array([0.3, 1.0, 0, 0, 0, 0, 0]))          # 1/240 > 1e-4: joint 1 is stopped, joint 0 is not
    assert s[1] == hi and s[7 + 1] == 0.0 and s[7] == 0.3
    s, _, _ = env.step(np.array([0, -1.0, 0, 0, 0, 0, 0]))
    assert s[1] == hi - 1.0 / 240.0 and s[7 + 1] == -1.0
    cont = env_of("standin8")                                         # continuous joints have no limits
    cont.q[:] = 100.0
    assert cont.step(np.ones(8))[0][0] == 100.0 + 1.0 / 240.0
    assert not any(j.limited for j in cont.model.joints)


def test_protocol_pickling_and_host_vector_env_factory():
    import functools
    ee, involved, fixed, init, var = ARMS["iiwa_like7"]
    factory = functools.partial(build_kinematic, path("iiwa_like7"), ee, fixed, involved, [0.4, 0.2, 0.6], [0.3, 0.1, 0.5], init, var)
    env = factory()
    assert env.observation_space.shape == (23,) and env.action_space.shape == (7,)
    assert list(env.target_pos) == [0.4, 0.2, 0.6] and list(env.obstacle_pos) == [0.3, 0.1, 0.5]
    assert env.initial_positions_variation_range == var
    s = env.reset(verbose=False)
    assert s.shape == (23,) and s.dtype == np.float64
    s2, r, done = env.step(np.full(7, 0.1))
    assert s2.shape == (23,) and done in (0, 1) and isinstance(r, float)
    np.testing.assert_array_equal(s2[14:17], env.end_effector())
    np.testing.assert_array_equal(s2[17:20], [0.4, 0.2, 0.6])
    np.testing.assert_array_equal(s2[20:23], [0.3, 0.1, 0.5])
    clone = pickle.loads(pickle.dumps(env))
    np.testing.assert_array_equal(clone.step(np.full(7, 0.2))[0], env.step(np.full(7, 0.2))[0])
    pickle.loads(pickle.dumps(factory))
    from robotic_manipulator_rloa_amd.environment.vector_env import HostVectorEnv
    vec = HostVectorEnv(factory, 2, 23, 7, max_frames=5, seed=0)
    try:
        obs = vec.reset()
        assert np.asarray(obs).shape == (2, 23)
        out = vec.step(np.zeros((2, 7), np.float32))
        np.testing.assert_allclose(np.asarray(out[-1])[:, 17:20], [[0.4, 0.2, 0.6]] * 2, atol=1e-6)
    finally:
        vec.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, words", [("bad_planar", "planar"), ("bad_two_roots", "root"), ("bad_truncated", "malformed XML")])
def test_bad_files_are_refused_with_the_cause(name, words):
    with pytest.raises(InvalidManipulatorFile, match=words):
        UC.load_urdf(path(name))


def test_other_refusals_name_the_cause(tmp_path):
    with pytest.raises(InvalidManipulatorFile, match="not found"):
        UC.load_urdf(str(tmp_path / "nothing.urdf"))
    sdf = tmp_path / "kuka_with_gripper2.sdf"
    sdf.write_text("<sdf/>")
    with pytest.raises(InvalidManipulatorFile, match=r"\.sdf"):
        UC.load_urdf(str(sdf))
    # a branching involved_joints: the two fingers are siblings, neither is above the other
    with pytest.raises(InvalidManipulatorFile, match="finger_right_joint"):
        model_of("arm_with_gripper", involved_joints=[1, 2, 3, 4, 5, 6, 8, 9], fixed_joints=[0, 7], endeffector_index=8)
    with pytest.raises(InvalidManipulatorFile, match="serial chain"):
        model_of("planar3", involved_joints=[1, 0, 2])
    with pytest.raises(InvalidManipulatorFile, match="65 involved joints"):
        model_of("long32", involved_joints=list(range(65)))
    with pytest.raises(InvalidManipulatorFile, match="cannot be driven"):
        model_of("arm_with_gripper", involved_joints=[0, 1, 2])
    with pytest.raises(InvalidManipulatorFile, match="joint index 40"):
        model_of("long32", endeffector_index=40)
    with pytest.raises(InvalidManipulatorFile, match="does not descend"):
        model_of("arm_with_gripper", involved_joints=[3, 4], endeffector_index=1)


# ---- 6. the blob -------------------------------------------------------------------------------------------------------------
def blob_end_effector(blob, q):
    """A numpy reader of the layout include/naf_hip.h documents (float32 blob, float64 arithmetic)."""
    b = blob.astype(np.float64)
    assert b[0] == 1
    A, n_seg, ee_frame = int(b[1]), int(b[2]), int(b[4])
    assert b[8] == b.size == 16 + 24 * A + (A + 2) + 8 * n_seg + 2 * A
    R, p = np.eye(3), np.zeros(3)
    frames = [(R, p)]
    for k in range(A):
        j = b[16 + 24 * k:16 + 24 * (k + 1)]
        p = p + R @ j[9:12]
        R = R @ j[0:9].reshape(3, 3)
        x, y, z = j[12:15]
        if j[15] == 1:
            p = p + R @ j[12:15] * q[k]
        else:
            K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
            R = R @ (np.eye(3) + np.sin(q[k]) * K + (1 - np.cos(q[k])) * K @ K)
        frames.append((R, p))
    R, p = frames[ee_frame]
    return p + R @ b[5:8]


@pytest.mark.parametrize("name", list(ARMS))
def test_pack_round_trip_and_model_check(name):
    from robotic_manipulator_rloa_amd import _lib
    lib = _lib.load()
    m = model_of(name)
    env = KinematicEnvironment(m, (0, 0, 0), (5, 5, 5))
    blob = m.pack()
    assert blob.dtype == np.float32 and blob.ndim == 1
    rng = np.random.default_rng(3)
    for _ in range(50):
        q = random_q(m, rng)
        np.testing.assert_allclose(blob_end_effector(blob, q), env.end_effector(q), atol=16 * m.A * 2.0 ** -24 * m.reach)
    check = lambda b: lib.naf_chain_env_model_check(b.ctypes.data, int(b.size))      # noqa: E731
    assert check(blob) == 0
    import hashlib
    assert m.digest() == hashlib.sha256(blob.tobytes()).hexdigest() and len(m.digest()) == 64
    travel = sum(max(abs(j.lower), abs(j.upper)) for j in m.joints if j.type == UC.PRISMATIC and j.limited)      # (slider4's 0.4 + 0.3)
    assert abs(m.reach - (sum(np.linalg.norm(j.pre_xyz) for j in m.joints) + np.linalg.norm(m.ee_point) + travel)) < 1e-12
    bad = blob.copy()
    bad[0] = 2
    assert check(bad) == -11                                  # NAF_CHAIN_ERR_VERSION
    cut = np.ascontiguousarray(blob[:-3])
    assert check(cut) == -12                                  # NAF_CHAIN_ERR_SIZE
    assert lib.naf_chain_env_model_check(blob.ctypes.data, 8) == -1 and lib.naf_chain_env_model_check(None, 100) == -1
    A, n_seg = m.A, len(m.segments)
    seg0 = 16 + 24 * A + A + 2
    frames = blob[seg0:seg0 + 8 * n_seg:8]
    assert list(frames) == sorted(frames)
    i = int(np.nonzero(np.diff(frames))[0][0])                # swap two neighbouring segments of different frames
    uns = blob.copy()
    uns[seg0 + 8 * i:seg0 + 8 * (i + 1)], uns[seg0 + 8 * (i + 1):seg0 + 8 * (i + 2)] = \
        blob[seg0 + 8 * (i + 1):seg0 + 8 * (i + 2)], blob[seg0 + 8 * i:seg0 + 8 * (i + 1)]
    assert check(uns) == -17                                  # NAF_CHAIN_ERR_SEGMENTS
    nan = blob.copy()
    nan[20] = np.nan
    assert check(nan) == -14
    ax = blob.copy()
    ax[16 + 12:16 + 15] = [0.5, 0.5, 0.0]                     # not a unit axis
    assert check(ax) == -16
    out = ctypes.c_void_p()
    assert lib.naf_chain_env_create(bad.ctypes.data, int(bad.size), ctypes.byref(out)) == -11 and not out.value
    assert lib.naf_chain_env_state_floats(None) == -1 and lib.naf_chain_env_destroy(None) == -1
    assert lib.naf_chain_env_step(None, None, None, None, None, 1, 0, None, 0, None, 0, None) == -1
    assert lib.naf_chain_env_reset(None, None, None, 1, None, 0, 0, None) == -1


def test_the_header_states_the_layout_the_packer_uses():
    from robotic_manipulator_rloa_amd import _lib
    import re
    header = open(os.path.join(_lib.CSRC, "..", "..", "include", "naf_hip.h")).read()
    value = lambda n: int(re.search(rf"#define {n} \(?(-?\d+)\)?", header).group(1))      # noqa: E731
    assert value("NAF_CHAIN_BLOB_VERSION") == UC.BLOB_VERSION and value("NAF_CHAIN_HEADER_FLOATS") == UC.HEADER_FLOATS
    assert value("NAF_CHAIN_JOINT_FLOATS") == UC.JOINT_FLOATS and value("NAF_CHAIN_SEGMENT_FLOATS") == UC.SEGMENT_FLOATS
    assert _lib.header_abi_version() >= 36 and "chain_env.hip" in _lib.SOURCES


# ---- 7. framework plumbing without a device ---------------------------------------------------------------------------------
def test_framework_kinematic_environment_without_a_gpu(monkeypatch):
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.utils.exceptions import EnvironmentNotInitialized
    ee, involved, fixed, init, var = ARMS["arm_with_gripper"]
    f = ManipulatorFramework()
    with pytest.raises(EnvironmentNotInitialized):
        f.initialize_naf_agent()
    with pytest.raises(InvalidManipulatorFile, match="visualize"):
        f.initialize_kinematic_environment(path("arm_with_gripper"), ee, fixed, involved, [0.3, 0.2, 0.4], [0.2, 0.1, 0.3], visualize=True)
    with pytest.raises(InvalidManipulatorFile, match=r"\.sdf"):
        f.initialize_kinematic_environment("kuka_iiwa/kuka_with_gripper2.sdf", 13, [], [0], [0, 0, 0], [1, 1, 1])
    assert f.env is None
    f.initialize_kinematic_environment(path("arm_with_gripper"), ee, fixed, involved, [0.3, 0.2, 0.4], [0.2, 0.1, 0.3], init, var,
                                       link_radius=0.02, obstacle_radius=0.07, obstacle_jitter=0.01, max_force=50.)
    assert isinstance(f.env, KinematicEnvironment) and f.env.observation_space.shape == (21,) and f.env.action_space.shape == (6,)
    kw = f._device_env_arguments()
    assert kw["chain"] is f.env.model and kw["scene"] == {"target": [0.3, 0.2, 0.4], "obstacle": [0.2, 0.1, 0.3],
                                                           "obstacle_radius": 0.07, "obstacle_jitter": 0.01}
    twin = f._env_factory()
    assert isinstance(twin, KinematicEnvironment) and twin.model.digest() == f.env.model.digest()

    class Agent:                      # records what the framework forwards; no device behind it
        state_size, action_size, seed = 21, 6, 0
        calls = []

        def run(self, frames, episodes, verbose, **kw):
            self.calls.append(("run", frames, episodes, kw))
            return {}

        def run_vectorized(self, *a, **kw):
            self.calls.append(("run_vectorized", a, kw))
            return {"scores": {1: (0.0, 1)}}

        def evaluate_vectorized(self, n, frames, **kw):
            self.calls.append(("evaluate_vectorized", n, frames, kw))
            return [(True, 3, True)] * n

    f.naf_agent = Agent()
    f.run_training(3, 50, verbose=False)
    assert Agent.calls[-1][:3] == ("run", 50, 3)
    assert f.run_training(3, 50, verbose=False, n_envs=4) == {1: (0.0, 1)}
    name, a, kw = Agent.calls[-1]
    assert name == "run_vectorized" and kw["chain"] is f.env.model and kw["n_envs"] == 4 and kw["max_frames"] == 50 and \
        kw["scene"]["obstacle_radius"] == 0.07 and "preset" not in kw
    f.run_vectorized_training(10, n_envs=8, max_frames=20)
    assert Agent.calls[-1][2]["chain"] is f.env.model
    out = f.test_trained_model(4, 30, n_envs=2)
    assert Agent.calls[-1][0] == "evaluate_vectorized" and Agent.calls[-1][3]["chain"] is f.env.model
    assert out["successes"] == 4 and out["episodes"] == 4
    f.delete_environment()
    assert f.env is None and f._env_factory is None


def test_scene_and_chain_travel_together():
    from robotic_manipulator_rloa_amd.naf_components.naf_algorithm import NAFAgent
    m = model_of("planar3")
    assert NAFAgent._chain_arguments(None, None) == {}
    with pytest.raises(ValueError, match="chain"):
        NAFAgent._chain_arguments(None, {"target": [0, 0, 0], "obstacle": [1, 1, 1]})
    with pytest.raises(ValueError, match="scene"):
        NAFAgent._chain_arguments(m, None)
    with pytest.raises(ValueError, match="unknown"):
        NAFAgent._chain_arguments(m, {"target": [0, 0, 0], "obstacle": [1, 1, 1], "radius": 1})
    kw = NAFAgent._chain_arguments(m, {"target": [0, 0, 0], "obstacle": [1, 1, 1]})
    assert kw["chain"] is m and kw["obstacle_radius"] == 0.06 and kw["obstacle_jitter"] == 0.0
