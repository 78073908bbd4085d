"""CPU (`-m "not gpu"`): the kinematic environment's self-collision rule — which capsule pairs the compiler tests
(environment/urdf_chain.py), the segment-segment distance and the reward rule of the float64 twin (environment/kinematic.py),
the pruning of pairs that are always in contact, the pair table of the blob and the library's check of it, and a float32
rehearsal of the kernel's pair arithmetic on the inputs of the GPU test."""
import ctypes
import functools
import pickle

import numpy as np
import pytest

from test_chain_env_cpu import ARMS, model_of, path, random_q

from robotic_manipulator_rloa_amd.environment import urdf_chain as UC
from robotic_manipulator_rloa_amd.environment.kinematic import (KinematicEnvironment, build_kinematic, segment_point_distance2,
                                                                segment_segment_distance2)
from robotic_manipulator_rloa_amd.utils.exceptions import InvalidManipulatorFile

SELFCOL_ARMS = ["planar3", "iiwa_like7", "arm_with_gripper", "standin8", "long12", "long32"]
FAR = (50.0, 50.0, 50.0)


def selfcol_model(name, **over):
    return model_of(name, consider_autocollision=True, **over)


def scattered_q(name, E, n, seed=11):
    """The scattered configurations of the GPU kernel-against-twin test: n batches of E poses, float32, uniform inside the limits."""
    model = selfcol_model(name)
    rng = np.random.default_rng(seed)
    return model, [np.stack([random_q(model, rng) for _ in range(E)]).astype(np.float32) for _ in range(n)]


# ---- 1. the pair rule ------------------------------------------------------------------------------------------------------
def test_pair_rule_written_out_by_hand():
    """arm_with_gripper, joints in file order (= PyBullet's indices): 0 world_joint (fixed) world -> base, 1 .. 6 joint1 .. joint6
    base -> link1 -> .. -> link6, 7 gripper_fix link6 -> gripper_base, 8 / 9 the finger joints gripper_base -> finger_left /
    finger_right. Link k is joint k's child, so base = 0, link1 .. link6 = 1 .. 6, gripper_base = 7, finger_left = 8,
    finger_right = 9 and the root `world` = -1. One capsule per (link, child joint) plus the end-effector link's own: world 1,
    base 1, link1 .. link6 1 each, gripper_base 3 (to either finger joint and to its centre of mass); the fingers have no child
    and carry none. Tested link pairs: i, j in 0 .. 7, |i - j| > 1: 28 - 7 = 21, of which 6 have gripper_base (j = 7, i = 0 .. 5),
    three capsules each: 15 + 18 = 33 segment pairs."""
    m = selfcol_model("arm_with_gripper")
    assert [(s.link, s.link_name) for s in m.segments] == [
        (-1, "world"), (0, "base"), (1, "link1"), (2, "link2"), (3, "link3"), (4, "link4"), (5, "link5"), (6, "link6"),
        (7, "gripper_base"), (7, "gripper_base"), (7, "gripper_base")]
    link = [s.link for s in m.segments]
    want = [(s, t) for s in range(11) for t in range(s + 1, 11) if link[s] >= 0 and link[t] >= 0 and abs(link[s] - link[t]) > 1]
    assert len(want) == 33
    kept = set(m.self_pairs)
    dropped_links = set(m.self_pairs_dropped)
    assert kept <= set(want) and len(kept) + len(m.self_pairs_dropped) == 33
    for s, t in want:
        assert (s, t) in kept or (m.segments[s].link_name, m.segments[t].link_name) in dropped_links
    for s, t in kept:
        assert s < t and link[s] >= 0 and abs(link[s] - link[t]) > 1          # never the root, never neighbours
    assert not any(0 in p for p in kept)                                      # segment 0 is the root link's
    assert (1, 2) not in kept and (7, 8) not in kept and (8, 9) not in kept   # neighbours / the same link
    # planar3: base (root) | l1 = 0, l2 = 1, l3 = 2: the one tested pair is l1 against l3
    p = selfcol_model("planar3")
    assert [(s.link, s.link_name) for s in p.segments] == [(-1, "base"), (0, "l1"), (1, "l2"), (2, "l3")]
    assert p.self_pairs == [(1, 3)] and p.self_pairs_dropped == []
    # off: nothing is carried
    off = model_of("arm_with_gripper")
    assert off.self_pairs == [] and off.self_pairs_dropped == [] and not off.consider_autocollision
    assert [s.link for s in off.segments] == link


# ---- 2. segment-segment distance ---------------------------------------------------------------------------------------------
def d_of(a1, b1, a2, b2):
    return float(np.sqrt(segment_segment_distance2(*(np.array(v, float) for v in (a1, b1, a2, b2)))))


def test_segment_distance_hand_worked_degenerate_cases():
    assert d_of((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)) == 1.0                      # parallel, side by side
    assert d_of((0, 0, 0), (1, 0, 0), (3, 1, 0), (5, 1, 0)) == pytest.approx(np.sqrt(5.0), abs=1e-15)   # parallel, apart: end to end
    assert d_of((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)) == 1.0                      # collinear, apart
    assert d_of((0, 0, 0), (2, 0, 0), (1, 0, 0), (3, 0, 0)) == 0.0                      # collinear, overlapping
    assert d_of((0, 0, 0), (2, 0, 0), (0.5, 0, 0), (1.5, 0, 0)) == 0.0                  # one inside the other
    assert d_of((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)) == 0.0                    # crossing
    assert d_of((-1, 0, 0), (1, 0, 0), (0, -1, 0.25), (0, 1, 0.25)) == 0.25             # skew: the lines' closest points, interior
    assert d_of((0, 0, 0), (1, 0, 0), (2, 1, 0), (2, 3, 0)) == pytest.approx(np.sqrt(2.0), abs=1e-15)   # end point to end point
    assert d_of((0, 0, 0), (1, 0, 0), (0.5, 2, 0), (0.5, 1, 0)) == 1.0                  # end point to interior
    assert d_of((0.25, 3, 4), (0.25, 3, 4), (0, 0, 0), (1, 0, 0)) == 5.0                # zero length, first
    assert d_of((0, 0, 0), (1, 0, 0), (0.25, 3, 4), (0.25, 3, 4)) == 5.0                # zero length, second
    assert d_of((1, 2, 3), (1, 2, 3), (1, 2, 5), (1, 2, 5)) == 2.0                      # both
    assert d_of((1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 2, 3)) == 0.0
    assert d_of((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1 + 1e-9, 0)) == pytest.approx(1.0, abs=1e-12)     # nearly parallel
    # batched: leading dimensions broadcast
    a1 = np.zeros((4, 3))
    b1 = np.tile([1.0, 0, 0], (4, 1))
    a2 = np.array([[0, k, 0] for k in range(4)], float)
    np.testing.assert_array_equal(segment_segment_distance2(a1, b1, a2, a2 + [1.0, 0, 0]), [0.0, 1.0, 4.0, 9.0])


def test_segment_distance_against_a_brute_force_grid():
    """200 random pairs (some nearly parallel, some short): the minimum over a 2001 x 2001 grid of the two parameters is never
    below the true distance, and exceeds it by at most half a grid step along each segment: (|d1| + |d2|) / 4000 <=
    max(|d1|, |d2|) / 2000, the grid's own resolution."""
    rng = np.random.default_rng(8)
    g = np.linspace(0.0, 1.0, 2001)
    for k in range(200):
        a1, a2 = rng.normal(size=3), rng.normal(size=3) * 0.5
        d1 = rng.normal(size=3) * rng.choice([1.0, 0.05])
        d2 = rng.normal(size=3) if k % 4 else d1 * rng.uniform(-2, 2) + rng.normal(size=3) * 1e-3
        w = a1 - a2
        A, B, C, D, E = d1 @ d1, d1 @ d2, d2 @ d2, d1 @ w, d2 @ w
        grid = w @ w + (A * g * g + 2 * D * g)[:, None] + (C * g * g - 2 * E * g)[None, :] - 2 * B * np.outer(g, g)
        brute = np.sqrt(max(grid.min(), 0.0))
        got = d_of(a1, a1 + d1, a2, a2 + d2)
        res = max(np.linalg.norm(d1), np.linalg.norm(d2)) / 2000
        assert got <= brute + 1e-9 and brute - got <= res, (k, got, brute, res)


# ---- 3. the rule in the twin ---------------------------------------------------------------------------------------------------
THETA = np.pi - np.arcsin(0.84)


def test_planar3_folded_onto_itself():
    """q0 = 0: l1 lies on the x axis from 0 to 0.3. q1 = theta bends l2 (0.25 long) back over it, q2 = 3 pi / 2 - theta points l3
    (0.15 long) straight down at l1. Its tip is then 0.25 sin(theta) - 0.15 above l1 (and over it: x = 0.3 + 0.25 cos(theta), 0.164
    at the threshold), so with capsule radii 0.03 + 0.03 the pair touches when 0.25 sin(theta) - 0.15 = 0.06: theta* = pi -
    asin(0.84). Around theta*, with q2 held, the clearance falls at 0.25 |cos(theta*)| = 0.1356 per radian."""
    q2 = 1.5 * np.pi - THETA
    half = 0.5 / 240.0
    far = np.array(FAR)
    on = KinematicEnvironment(selfcol_model("planar3"), far, far)
    off = KinematicEnvironment(model_of("planar3"), far, far)
    assert on.self_clearance(np.array([0.0, THETA, q2])) == pytest.approx(0.0, abs=1e-15)
    assert off.self_clearance(np.array([0.0, THETA, q2])) == np.inf and off.self_clearance(np.zeros((5, 3))).shape == (5,)
    rate = 0.25 * abs(np.cos(THETA))
    for env in (on, off):
        env.q = np.array([0.0, THETA - 3 * half, q2])
        s, r, done = env.step(np.array([0.0, 1.0, 0.0]))                  # to theta* - 1/480: one step before the threshold
        dist = np.linalg.norm(s[6:9] - far)
        assert done == 0 and r == pytest.approx(-(dist - 0.05), abs=1e-12)
        if env is on:
            assert env.last_self_clearance == pytest.approx(rate * half, rel=0.02) and env.last_self_clearance > 0
        s, r, done = env.step(np.array([0.0, 1.0, 0.0]))                  # to theta* + 1/480: across it
        if env is on:
            assert (r, done) == (-1000, 1)
            assert env.last_self_clearance == pytest.approx(-rate * half, rel=0.02) and env.last_clearance > 1.0
        else:
            assert done == 0 and r == pytest.approx(-(np.linalg.norm(s[6:9] - far) - 0.05), abs=1e-12)
            assert env.last_self_clearance == np.inf
    # reaching the target wins over self-contact (environment.py:345-371 tests the target first)
    deep = np.array([0.0, THETA + 0.2, q2])
    on.q = deep.copy()
    on.target_pos = on.end_effector(deep)
    assert on.self_clearance(deep) < -0.01 and on.step(np.zeros(3))[1:] == (250, 1)
    # obstacle contact and self-contact together are one -1000
    on.q = deep.copy()
    on.target_pos, on.obstacle_pos = far, on.end_effector(deep)
    assert on.step(np.zeros(3))[1:] == (-1000, 1) and on.last_clearance < on.obstacle_radius and on.last_self_clearance < 0
    # batched as clearance() is
    q = np.stack([[0.0, THETA - 0.01, q2], [0.0, THETA + 0.01, q2]])
    c = on.self_clearance(q)
    assert c.shape == (2,) and c[0] > 0 > c[1]
    assert on.pair_clearances(q).shape == (1, 2)


# ---- 4. pruning, exceptions by hand, the start pose ---------------------------------------------------------------------------
@pytest.mark.parametrize("name, tested, dropped", [("iiwa_like7", 20, 2), ("arm_with_gripper", 33, 5), ("standin8", 21, 3),
                                                   ("planar3", 1, 0), ("long12", 55, 0), ("long32", 465, 0)])
def test_pairs_always_in_contact_are_dropped(name, tested, dropped):
    m = selfcol_model(name)
    assert len(m.self_pairs_dropped) == dropped and len(m.self_pairs) == tested - dropped
    again = selfcol_model(name)
    assert again.self_pairs == m.self_pairs and again.self_pairs_dropped == m.self_pairs_dropped and again.digest() == m.digest()
    assert all(isinstance(a, str) and isinstance(b, str) for a, b in m.self_pairs_dropped)
    # what was dropped IS in contact at every pose of another sample, what was kept is not
    twin = KinematicEnvironment(m, FAR, FAR)
    rng = np.random.default_rng(123)
    q = np.stack([random_q(m, rng) for _ in range(500)])
    assert np.all(np.any(twin.pair_clearances(q) >= 0.0, axis=1))
    full = selfcol_model(name)
    link = [s.link for s in m.segments]
    full.self_pairs = [(s, t) for s in range(len(link)) for t in range(s + 1, len(link))
                       if min(link[s], link[t]) >= 0 and abs(link[s] - link[t]) > 1 and (s, t) not in set(m.self_pairs)]
    if dropped:
        assert len(full.self_pairs) == dropped and np.all(KinematicEnvironment(full, FAR, FAR).pair_clearances(q) < 0.0)
    if name == "standin8":                                    # each bridges one short link: two links apart
        names = [j.child for j in UC.load_urdf(path(name)).joints]
        assert all(abs(names.index(a) - names.index(b)) == 2 for a, b in m.self_pairs_dropped)
    assert UC.SELF_PRUNE_POSES == 256 and isinstance(UC.SELF_PRUNE_SEED, int)


def test_autocollision_ignore_and_the_start_pose_refusal():
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    base = selfcol_model("arm_with_gripper")
    by_name = selfcol_model("arm_with_gripper", autocollision_ignore=[("base", "gripper_base")])
    by_index = selfcol_model("arm_with_gripper", autocollision_ignore=[(7, 0)])
    gone = [(s, t) for s, t in base.self_pairs if {base.segments[s].link, base.segments[t].link} == {0, 7}]
    assert len(gone) == 3 and by_name.self_pairs == [p for p in base.self_pairs if p not in gone] == by_index.self_pairs
    assert by_name.digest() == by_index.digest() != base.digest()
    assert selfcol_model("arm_with_gripper", autocollision_ignore=[("finger_left", 2)]).self_pairs == base.self_pairs  # (no capsule)
    with pytest.raises(InvalidManipulatorFile, match="wrist"):
        selfcol_model("arm_with_gripper", autocollision_ignore=[("wrist", "base")])
    with pytest.raises(InvalidManipulatorFile, match="world"):                # the root link takes no part
        selfcol_model("arm_with_gripper", autocollision_ignore=[("world", "link3")])
    with pytest.raises(InvalidManipulatorFile, match="link index 10"):
        selfcol_model("arm_with_gripper", autocollision_ignore=[(10, 2)])
    with pytest.raises(InvalidManipulatorFile, match="pair of links"):
        selfcol_model("arm_with_gripper", autocollision_ignore=["base"])
    # the framework call refuses a start pose in self-contact and names the way out
    ee, involved, fixed, init, var = ARMS["planar3"]
    f = ManipulatorFramework()
    folded = [0.0, THETA + 0.2, 1.5 * np.pi - THETA]
    with pytest.raises(ValueError, match=r"'l1' and 'l3'.*clearance -0\.0\d+ m.*autocollision_ignore"):
        f.initialize_kinematic_environment(path("planar3"), ee, fixed, involved, [0.3, 0.2, 0.0], FAR, folded, var, link_radius=0.03,
                                           consider_autocollision=True)
    assert f.env is None
    f.initialize_kinematic_environment(path("planar3"), ee, fixed, involved, [0.3, 0.2, 0.0], FAR, folded, var, link_radius=0.03,
                                       consider_autocollision=True, autocollision_ignore=[("l1", "l3")])
    assert f.env.model.consider_autocollision and f.env.model.self_pairs == []
    f.initialize_kinematic_environment(path("planar3"), ee, fixed, involved, [0.3, 0.2, 0.0], FAR, folded, var, link_radius=0.03)
    assert not f.env.model.consider_autocollision                             # off: no refusal
    f.initialize_kinematic_environment(path("planar3"), ee, fixed, involved, [0.3, 0.2, 0.0], FAR, init, var, link_radius=0.03,
                                       consider_autocollision=True)
    assert f.env.model.self_pairs == [(1, 3)]
    assert f._device_env_arguments()["chain"] is f.env.model                  # the model carries the setting to the device loop
    twin = pickle.loads(pickle.dumps(f._env_factory))()                       # ... and the factory to the host vector env
    assert twin.model.self_pairs == [(1, 3)] and twin.model.digest() == f.env.model.digest()
    # long12's start pose is in contact by a millimetre or two: refused through the framework, compiled by compile_chain
    ee, involved, fixed, init, var = ARMS["long12"]
    with pytest.raises(ValueError, match="self-contact"):
        f.initialize_kinematic_environment(path("long12"), ee, fixed, involved, [0.3, 0.2, 0.4], FAR, init, var, link_radius=0.03,
                                           consider_autocollision=True)
    m = selfcol_model("long12")
    assert -0.003 < KinematicEnvironment(m, FAR, FAR).self_clearance(np.array([j.init for j in m.joints])) < 0.0
    env = build_kinematic(path("planar3"), 2, [], [0, 1, 2], [0.3, 0.2, 0.0], FAR, None, None, 0.03, 0.06, True, [("l1", "l3")])
    assert env.model.consider_autocollision and env.model.self_pairs == []
    pickle.loads(pickle.dumps(functools.partial(build_kinematic, path("planar3"), 2, [], [0, 1, 2], [0, 0, 0], FAR,
                                                consider_autocollision=True)))().step(np.zeros(3))


# ---- 5. the blob -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SELFCOL_ARMS)
def test_blob_with_and_without_the_pair_table(name):
    from robotic_manipulator_rloa_amd import _lib
    lib = _lib.load()

    def check(b):
        b = np.ascontiguousarray(b)
        return lib.naf_chain_env_model_check(b.ctypes.data, int(b.size))
    plain, off, on = model_of(name), model_of(name, consider_autocollision=False), selfcol_model(name)
    assert off.pack().tobytes() == plain.pack().tobytes() and off.digest() == plain.digest()
    base = plain.pack()
    assert base[9] == 0 and np.all(base[10:16] == 0)
    blob = on.pack()
    P = len(on.self_pairs)
    assert P > 0 and blob[9] == P and blob[8] == blob.size == base.size + 2 * P and on.digest() != plain.digest()
    head = blob[:base.size].copy()
    head[8], head[9] = base[8], 0
    assert head.tobytes() == base.tobytes()                                    # nothing else moved
    np.testing.assert_array_equal(blob[base.size:].reshape(P, 2), np.array(on.self_pairs, np.float32))
    assert check(blob) == 0 and check(base) == 0
    n_seg = len(on.segments)

    def with_pair(k, s, t):
        b = blob.copy()
        b[base.size + 2 * k:base.size + 2 * k + 2] = [s, t]
        return b
    s0, t0 = on.self_pairs[0]
    assert check(with_pair(0, s0, n_seg)) == -19                               # out of range
    assert check(with_pair(0, -1, t0)) == -19
    assert check(with_pair(0, t0, s0)) == -19 and check(with_pair(0, s0, s0)) == -19      # s >= t
    assert check(with_pair(0, s0, t0 + 0.5)) == -19                            # not an integer
    if P > 1:
        assert check(with_pair(0, *on.self_pairs[1])) == -19                   # a pair twice
    cut = blob[:-2].copy()                                                     # the table one pair short of the count in [9]
    cut[8] = cut.size
    assert check(cut) == -19
    more = blob.copy()
    more[9] = P + 1
    assert check(more) == -19
    claimed = base.copy()                                                      # pairs counted, no table
    claimed[9] = 1
    assert check(claimed) == -19
    frac = blob.copy()
    frac[9] = P + 0.5
    assert check(frac) == -19
    assert check(blob[:-3]) == -12                                             # [8] against the length: NAF_CHAIN_ERR_SIZE
    v2 = blob.copy()
    v2[0] = 2
    assert check(v2) == -11                                                    # NAF_CHAIN_ERR_VERSION
    nan = blob.copy()
    nan[-1] = np.nan
    assert check(nan) == -14
    out = ctypes.c_void_p()
    assert lib.naf_chain_env_create(with_pair(0, t0, s0).ctypes.data, int(blob.size), ctypes.byref(out)) == -19 and not out.value
    assert lib.naf_chain_env_probe(None, None, None, 1, None) == -1
    assert _lib.header_abi_version() >= 37


# ---- 6. float32 rehearsal of the kernel's pair arithmetic ------------------------------------------------------------------------
def seg_point_dist2_f32(a, b, c):
    """seg_point_dist2 of csrc/chain_env.hip, operation by operation, in float32 (numpy rounds every operation; the compiler may
    contract a multiply-add, which is at least as exact)."""
    f = np.float32
    u, w = b - a, c - a
    den = u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1] + u[..., 2] * u[..., 2]
    dot = w[..., 0] * u[..., 0] + w[..., 1] * u[..., 1] + w[..., 2] * u[..., 2]
    t = np.where(den > 0, dot / np.where(den > 0, den, f(1)), f(0)).astype(f)
    t = np.minimum(f(1), np.maximum(f(0), t))
    d = w - t[..., None] * u
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def seg_seg_dist2_f32(a, b, c, d):
    """seg_seg_dist2 of csrc/chain_env.hip in float32."""
    f = np.float32
    dot = lambda x, y: x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]      # noqa: E731
    clamp = lambda x: np.minimum(f(1), np.maximum(f(0), x))                                         # noqa: E731
    u, v, w = b - a, d - c, a - c
    A, B, C, D, E = dot(u, u), dot(u, v), dot(v, v), dot(u, w), dot(v, w)
    den = A * C - B * B
    ok = den > f(1e-7) * A * C
    s = clamp(np.where(ok, (B * E - C * D) / np.where(ok, den, f(1)), f(0)).astype(f))
    t = clamp(np.where(C > 0, (B * s + E) / np.where(C > 0, C, f(1)), f(0)).astype(f))
    s = clamp(np.where(A > 0, (B * t - D) / np.where(A > 0, A, f(1)), f(0)).astype(f))
    x = w + s[..., None] * u - t[..., None] * v
    best = dot(x, x)
    for cand in (seg_point_dist2_f32(c, d, a), seg_point_dist2_f32(c, d, b), seg_point_dist2_f32(a, b, c), seg_point_dist2_f32(a, b, d)):
        best = np.minimum(best, cand)
    assert best.dtype == np.float32
    return best


@pytest.mark.parametrize("name", SELFCOL_ARMS)
def test_float32_rehearsal_of_the_pair_formula(name):
    """The band of the GPU test is 4 tol: 2 tol for the four end points of a pair (each within tol = 16 A 2^-24 reach of the
    twin's), 2 tol for the pair formula's own float32 rounding. Here the end points are the twin's, rounded to float32, so what
    is left is the formula alone, on the GPU test's own scattered poses (E = 64): it must stay within 2 tol."""
    model, batches = scattered_q(name, 64, 40)
    twin = KinematicEnvironment(model, FAR, FAR)
    tol = 16 * model.A * 2.0 ** -24 * model.reach
    q = np.concatenate(batches).astype(np.float64)
    segs = twin.world_segments(q)
    want = twin.self_clearance(q)
    got = np.full(q.shape[0], np.inf, np.float32)
    for s, t in model.self_pairs:
        a, b, c, d = (np.float32(x) for x in (segs[s][0], segs[s][1], segs[t][0], segs[t][1]))
        got = np.minimum(got, np.sqrt(seg_seg_dist2_f32(a, b, c, d)) - (np.float32(segs[s][2]) + np.float32(segs[t][2])))
    worst = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{name}: float32 pair formula against the twin: worst {worst:.3e}, 2 tol = {2 * tol:.3e}")
    assert worst <= 2 * tol, (worst, 2 * tol)


# ---- 7. arms with many capsules ---------------------------------------------------------------------------------------------------
def spiky_model(tmp_path, stubs_per_link, **over):
    """planar3's chain (driven joints 0 .. 2 first, so l1 .. l3 are links 0 .. 2) with `stubs_per_link` short side branches on
    every link: fixed joints to leaf links, one capsule each, all belonging to the link they grow from."""
    lengths = [0.3, 0.25, 0.15]
    out = ['<?xml version="1.0"?>', '<robot name="spiky">', '<link name="base"/>']
    out += [f'<link name="l{k + 1}"/>' for k in range(3)]
    parents = ["base", "l1", "l2"]
    for k in range(3):
        out.append(f'<joint name="j{k}" type="revolute"><parent link="{parents[k]}"/><child link="l{k + 1}"/>'
                   f'<origin xyz="{0.0 if k == 0 else lengths[k - 1]} 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/>'
                   '<limit lower="-3.1416" upper="3.1416" effort="100" velocity="10"/></joint>')
    for k in range(3):
        for i in range(stubs_per_link):
            x = lengths[k] * (i + 0.5) / stubs_per_link
            y, z = 0.02 * np.cos(2.4 * i), 0.02 * np.sin(2.4 * i)
            out.append(f'<link name="s{k}_{i}"/>')
            out.append(f'<joint name="f{k}_{i}" type="fixed"><parent link="l{k + 1}"/><child link="s{k}_{i}"/>'
                       f'<origin xyz="{x:.6f} {y:.6f} {z:.6f}" rpy="0 0 0"/></joint>')
    out.append("</robot>")
    file = tmp_path / f"spiky{stubs_per_link}.urdf"
    file.write_text("\n".join(out))
    kw = dict(endeffector_index=2, involved_joints=[0, 1, 2], fixed_joints=[], initial_joint_positions=[0.3, -0.4, 0.5],
              initial_positions_variation_range=[0.1, 0.1, 0.1], link_radius=0.01, consider_autocollision=True)
    kw.update(over)
    return UC.compile_chain(UC.load_urdf(str(file)), **kw)


def test_an_arm_whose_end_points_do_not_fit_is_refused_by_name(tmp_path):
    """create() keeps 24 bytes of LDS per capsule and env: 6,144 capsules fill a workgroup's 144 KiB with one env; more is
    NAF_CHAIN_ERR_LDS (-20), and only with pairs — without self-collision nothing is staged and the same arm is accepted."""
    from robotic_manipulator_rloa_amd import _lib
    lib = _lib.load()
    m = spiky_model(tmp_path, 2100, consider_autocollision=False)
    assert len(m.segments) == 3 + 3 * 2100 + 1
    plain = m.pack()
    assert lib.naf_chain_env_model_check(plain.ctypes.data, int(plain.size)) == 0
    m.self_pairs, m._blob = [(1, len(m.segments) - 1)], None
    blob = m.pack()
    assert lib.naf_chain_env_model_check(blob.ctypes.data, int(blob.size)) == 0
    out = ctypes.c_void_p()
    assert lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(out)) == -20 and not out.value
    small = spiky_model(tmp_path, 34)
    assert len(small.segments) == 106 and len(small.self_pairs) > 1000 and all(s < t for s, t in small.self_pairs)
