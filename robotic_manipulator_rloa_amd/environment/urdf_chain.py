"""URDF -> chain model of the kinematic environment (environment/kinematic.py on the host, csrc/chain_env.hip on the device).

Standard library + numpy only: no torch, no HIP. Line numbers cited as environment.py:N are the reference's
robotic_manipulator_rloa/environment/environment.py.

The model keeps the reference's environment RULE for the arm a URDF names — state layout, reward, terminal rule, velocity
control of the involved joints, held joints — with the commanded velocity applied exactly for one 1/240 s tick. It is NOT a
port of Bullet: no dynamics (gravity, motor force, solver), no mesh collision. Self-collision is the reference's rule between
the links' capsules, off by default (compile_chain(consider_autocollision=True), "self pairs" below).

  frames     frame 0 is the world (= the root link's frame: the base sits at the origin, environment.py:280-282); frame k + 1
             is the child link frame of driven joint k. Frame k + 1 = frame k . Pre_k . Motion_k(q_k), Pre_k being every constant
             transform between the two (joint origins, constant joints), folded here.
  segments   collision capsules, each in the frame of the last driven joint above it.
  slots      observation slot k of the A position / velocity slots reports joint INDEX k (environment.py:442-444).
  workcell   fixed geometry of the cell the arm stands in, the same in every episode: up to MAX_CELL spheres (cx, cy, cz, r),
             half-spaces (nx, ny, nz, d), n a unit vector, the free side n.x - d >= 0, and rounded oriented boxes (centre c, half
             extents h >= 0, orientation R, rounding radius r >= 0). Clearance of a capsule (world end points a, b, radius rho):
             distance(segment ab, c) - rho - r against a sphere, min(n.a, n.b) - d - rho against a half-space, distance(segment
             ab, box) - rho - r against a box (kinematic.segment_box_distance in the box's frame; 0 for a segment that enters
             the box: no penetration depth); contact when < 0, for the (capsule, geometry) pairs the model tests: reward -1000
             and done, as obstacle contact. Geometry index g counts the spheres first, then the half-spaces, then the boxes.
             Off unless compile_chain is given some.
  self pairs segment pairs (s, t), s < t, tested against each other when consider_autocollision is on: the reference tests
             link i against link j for i, j in 0 .. num_joints - 1 with |i - j| <= 1 left out, contact when the closest distance
             is below 0 (environment.py:311-343, :394-412; collision_detector.py:63-98). The root link (index -1) takes no part.
             Contact of a pair here: distance(segment s, segment t) - radius_s - radius_t < 0.
"""
from __future__ import annotations

import hashlib
import math
import os
import xml.etree.ElementTree as ET
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from ..utils.exceptions import InvalidManipulatorFile

# ---- blob layout (documented once, in include/naf_hip.h: "chain model blob") --------------------------------------------
BLOB_VERSION = 1
HEADER_FLOATS = 16
JOINT_FLOATS = 24
SEGMENT_FLOATS = 8
SLOT_FLOATS = 2
PAIR_FLOATS = 2
CELL_FLOATS = 4                  # per workcell sphere / half-space
BOX_FLOATS = 16                  # per workcell box, behind them: c (3) | R row-major (9) | h (3) | r; then one mask float per segment
MAX_CELL = 16                    # include/naf_hip.h NAF_CHAIN_MAX_CELL: spheres + half-spaces + boxes
MAX_JOINTS = 64
DT = 1.0 / 240.0                 # environment.py:481: one stepSimulation tick
TARGET_THRESHOLD = 0.05          # environment.py:345-371
OBSTACLE_RADIUS = 0.06           # the stand-in's (csrc/synth_env.hip)
SCENE_TRIES = 8                  # include/naf_hip.h NAF_CHAIN_SCENE_TRIES: candidate scenes per episode start
RANGE_FLOATS = 7                 # NAF_CHAIN_RANGE_FLOATS: target half-widths xyz | obstacle half-widths xyz | margin
# Capsules are fatter than meshes: a pair that is in contact at EVERY pose of this fixed sample (uniform inside the limits,
# +-pi where there are none) can never be out of contact and is dropped at compile time. Constants, so that one URDF always
# compiles to one model.
SELF_PRUNE_SEED = 20240607
SELF_PRUNE_POSES = 256
REVOLUTE, PRISMATIC = 0, 1
_MOVABLE = ("revolute", "continuous", "prismatic")


def rpy_matrix(rpy: Sequence[float]) -> np.ndarray:
    """URDF convention: R = Rz(yaw) . Ry(pitch) . Rx(roll)."""
    r, p, y = (float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def axis_rotation(axis: np.ndarray, q) -> np.ndarray:
    """Rodrigues: I + sin q . K + (1 - cos q) . K^2 for a unit axis; q a scalar or an array (one matrix per element)."""
    x, y, z = axis
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    q = np.asarray(q, float)[..., None, None]
    return np.eye(3) + np.sin(q) * K + (1.0 - np.cos(q)) * (K @ K)


@dataclass
class UrdfLink:
    name: str
    inertial_origin: Optional[np.ndarray] = None     # xyz of <inertial><origin>, None without <inertial>
    collision_radius: Optional[float] = None         # of a sphere / cylinder / capsule collision primitive


@dataclass
class UrdfJoint:
    name: str
    type: str
    parent: str
    child: str
    xyz: np.ndarray
    rot: np.ndarray
    axis: np.ndarray
    lower: float
    upper: float

    @property
    def limited(self) -> bool:
        return self.type != "continuous" and self.lower < self.upper


@dataclass
class Urdf:
    path: str
    links: Dict[str, UrdfLink]
    joints: List[UrdfJoint]      # FILE ORDER = PyBullet's joint index; joint k's child link is link index k
    root: str


def _floats(text: Optional[str], n: int, default: Sequence[float], what: str, path: str) -> np.ndarray:
    if text is None:
        return np.array(default, float)
    try:
        v = [float(t) for t in text.split()]
    except ValueError:
        v = []
    if len(v) != n or not all(math.isfinite(x) for x in v):
        raise InvalidManipulatorFile(f"{path}: {what} = {text!r} is not {n} finite numbers")
    return np.array(v, float)


def load_urdf(path: str) -> Urdf:
    if not str(path).lower().endswith(".urdf"):
        raise InvalidManipulatorFile(f"{path}: only .urdf files are read by the kinematic environment "
                                     f"(extension {os.path.splitext(str(path))[1] or 'missing'!r}; SDF is out of scope)")
    if not os.path.isfile(path):
        raise InvalidManipulatorFile(f"{path}: file not found")
    try:
        robot = ET.parse(path).getroot()
    except ET.ParseError as e:
        raise InvalidManipulatorFile(f"{path}: malformed XML ({e})") from e
    if robot.tag != "robot":
        raise InvalidManipulatorFile(f"{path}: the root element is <{robot.tag}>, not <robot>")
    links: Dict[str, UrdfLink] = {}
    for el in robot.findall("link"):
        link = UrdfLink(el.get("name", ""))
        inertial = el.find("inertial")
        if inertial is not None:
            o = inertial.find("origin")
            link.inertial_origin = _floats(None if o is None else o.get("xyz"), 3, (0, 0, 0),
                                           f"link {link.name} inertial origin xyz", path)
        for geom in el.findall("collision/geometry"):
            for kind in ("sphere", "cylinder", "capsule"):
                g = geom.find(kind)
                if g is not None and g.get("radius") is not None and link.collision_radius is None:
                    link.collision_radius = float(_floats(g.get("radius"), 1, (0,), f"link {link.name} {kind} radius", path)[0])
        links[link.name] = link
    joints: List[UrdfJoint] = []
    for el in robot.findall("joint"):
        name, jtype = el.get("name", ""), el.get("type", "")
        if jtype in ("floating", "planar"):
            raise InvalidManipulatorFile(f"{path}: joint {name!r} is of type {jtype}, which a kinematic chain cannot hold "
                                         "(revolute, continuous, prismatic and fixed are read)")
        if jtype not in _MOVABLE + ("fixed",):
            raise InvalidManipulatorFile(f"{path}: joint {name!r} has the unknown type {jtype!r}")
        parent, child = el.find("parent"), el.find("child")
        if parent is None or child is None or parent.get("link") not in links or child.get("link") not in links:
            raise InvalidManipulatorFile(f"{path}: joint {name!r} does not name a parent and a child among the links")
        o, a, lim = el.find("origin"), el.find("axis"), el.find("limit")
        axis = _floats(None if a is None else a.get("xyz"), 3, (1, 0, 0), f"joint {name} axis", path)
        norm = float(np.linalg.norm(axis))
        if jtype in _MOVABLE and norm < 1e-12:
            raise InvalidManipulatorFile(f"{path}: joint {name!r} has a zero axis")
        joints.append(UrdfJoint(
            name, jtype, parent.get("link"), child.get("link"),
            _floats(None if o is None else o.get("xyz"), 3, (0, 0, 0), f"joint {name} origin xyz", path),
            rpy_matrix(_floats(None if o is None else o.get("rpy"), 3, (0, 0, 0), f"joint {name} origin rpy", path)),
            axis / norm if norm >= 1e-12 else np.array([1.0, 0.0, 0.0]),
            float(_floats(None if lim is None else lim.get("lower"), 1, (0,), f"joint {name} lower limit", path)[0]),
            float(_floats(None if lim is None else lim.get("upper"), 1, (0,), f"joint {name} upper limit", path)[0])))
    children = {}
    for j in joints:
        if j.child in children:
            raise InvalidManipulatorFile(f"{path}: link {j.child!r} is the child of two joints")
        children[j.child] = j
    roots = [n for n in links if n not in children]
    if len(roots) != 1:
        raise InvalidManipulatorFile(f"{path}: {len(roots)} root links ({', '.join(sorted(roots)) or 'a cycle'}): "
                                     "a manipulator has exactly one")
    return Urdf(str(path), links, joints, roots[0])


@dataclass
class ChainJoint:
    index: int                   # URDF joint index
    pre_rot: np.ndarray          # Pre_k's rotation (3 x 3)
    pre_xyz: np.ndarray          # ... translation
    axis: np.ndarray
    type: int                    # REVOLUTE | PRISMATIC
    limited: bool
    lower: float
    upper: float
    init: float
    variation: float
    slot: int                    # observation slot that reports this joint (its URDF index when < A), else -1


@dataclass
class ChainSegment:
    frame: int
    a: np.ndarray
    b: np.ndarray
    radius: float
    link: int = -1               # PyBullet index of the link the capsule belongs to: the joint whose child it is; the root is -1
    link_name: str = ""


@dataclass
class ChainModel:
    joints: List[ChainJoint]
    segments: List[ChainSegment]             # sorted by frame
    ee_frame: int
    ee_point: np.ndarray
    slots: List[tuple]                       # per observation slot: (driven index or -1, constant value)
    reach: float                             # sum of the translation norms + the end-effector offset
    source: str = ""
    initial_positions_variation_range: Optional[List[float]] = None
    consider_autocollision: bool = False
    self_pairs: List[tuple] = field(default_factory=list)            # (s, t), s < t: segment indices tested against each other
    self_pairs_dropped: List[tuple] = field(default_factory=list)    # (link name, link name) of the pairs the pose sample pruned
    cell_spheres: List[tuple] = field(default_factory=list)          # (cx, cy, cz, r): geometry 0 .. G - 1
    cell_planes: List[tuple] = field(default_factory=list)           # (nx, ny, nz, d), |n| = 1, free side n.x - d >= 0: geometry G ..
    cell_boxes: List[tuple] = field(default_factory=list)            # 16 floats: c | R row-major | h | r: geometry G + H ..
    cell_masks: List[int] = field(default_factory=list)              # per segment: bit g set = tested against geometry g
    cell_pairs_dropped: List[tuple] = field(default_factory=list)    # (link name, geometry index) of the pairs the pose sample pruned
    _blob: Optional[np.ndarray] = field(default=None, repr=False, compare=False)

    @property
    def A(self) -> int:
        return len(self.joints)

    @property
    def state_size(self) -> int:
        return 2 * self.A + 9

    def segment_begin(self) -> List[int]:
        """begin[f] = index of frame f's first segment, f = 0 .. A + 1 (begin[A + 1] = the number of segments)."""
        frames = [s.frame for s in self.segments]
        return [int(np.searchsorted(frames, f, side="left")) for f in range(self.A + 2)]

    @property
    def n_cell(self) -> int:
        return len(self.cell_spheres) + len(self.cell_planes) + len(self.cell_boxes)

    @property
    def cell_pairs(self) -> List[tuple]:
        """(segment, geometry) pairs the workcell rule tests, segment-major."""
        return [(s, g) for s, mask in enumerate(self.cell_masks) for g in range(self.n_cell) if mask >> g & 1]

    def pack(self) -> np.ndarray:
        """The flat float32 blob csrc/chain_env.hip reads (layout: include/naf_hip.h, "chain model blob")."""
        if self._blob is not None:
            return self._blob.copy()
        A, n_seg, n_pairs = self.A, len(self.segments), len(self.self_pairs)
        head = np.zeros(HEADER_FLOATS)
        G, H, B = len(self.cell_spheres), len(self.cell_planes), len(self.cell_boxes)
        n = HEADER_FLOATS + JOINT_FLOATS * A + (A + 2) + SEGMENT_FLOATS * n_seg + SLOT_FLOATS * A + PAIR_FLOATS * n_pairs
        n += CELL_FLOATS * (G + H) + BOX_FLOATS * B + (n_seg if G + H + B else 0)      # (no workcell: the blob ends where it always did)
        head[:13] = [BLOB_VERSION, A, n_seg, A, self.ee_frame, *self.ee_point, n, n_pairs, G, H, B]
        parts = [head]
        for j in self.joints:
            rec = np.zeros(JOINT_FLOATS)
            rec[0:9], rec[9:12], rec[12:15] = j.pre_rot.reshape(9), j.pre_xyz, j.axis
            rec[15:22] = [j.type, 1.0 if j.limited else 0.0, j.lower, j.upper, j.init, j.variation, j.slot]
            parts.append(rec)
        parts.append(np.array(self.segment_begin(), float))
        for s in self.segments:
            parts.append(np.array([s.frame, *s.a, *s.b, s.radius]))
        for src, const in self.slots:
            parts.append(np.array([src, const]))
        for pair in self.self_pairs:                                  # (none: the blob is byte for byte the one without the table)
            parts.append(np.array(pair, float))
        for geom in list(self.cell_spheres) + list(self.cell_planes) + list(self.cell_boxes):
            parts.append(np.array(geom, float))
        if G + H + B:
            parts.append(np.array(self.cell_masks, float))
        self._blob = np.concatenate(parts).astype(np.float32)
        assert self._blob.size == n
        return self._blob.copy()

    def digest(self) -> str:
        return hashlib.sha256(self.pack().tobytes()).hexdigest()


def _compose(Ra, ta, Rb, tb):
    return Ra @ Rb, ta + Ra @ tb


def compile_chain(urdf: Urdf, endeffector_index: int, involved_joints: Sequence[int], fixed_joints: Sequence[int] = (),
                  initial_joint_positions: Optional[Sequence[float]] = None,
                  initial_positions_variation_range: Optional[Sequence[float]] = None, link_radius: float = 0.0,
                  consider_autocollision: bool = False, autocollision_ignore: Sequence = (), floor_height: Optional[float] = None,
                  workcell_planes: Optional[Sequence] = None, workcell_spheres: Optional[Sequence] = None,
                  cell_ignore: Sequence = (), workcell_boxes: Optional[Sequence] = None) -> ChainModel:
    """floor_height z0 (sugar for the half-space (0, 0, 1, z0), the first one), workcell_planes [(nx, ny, nz, d)],
    workcell_spheres [(cx, cy, cz, r)], workcell_boxes [(cx, cy, cz, hx, hy, hz)], [(.., roll, pitch, yaw)] or [(.., roll, pitch,
    yaw, r)] (half extents; the angles in rpy_matrix's convention; r the rounding radius — zero half extents with r > 0 give a
    fixed capsule or a rounded plate): the workcell (module text). The model tests every (capsule, geometry) pair except those
    the fixed pose sample finds in contact at every pose (listed in cell_pairs_dropped: the base standing on the floor) and
    those of cell_ignore: (link, geometry index) entries, the link by name or by PyBullet link index.
    consider_autocollision: the model carries self_pairs (module text) minus the pairs that the fixed pose sample finds in
    contact at every pose (listed in self_pairs_dropped) and minus autocollision_ignore: pairs of links, each given by name or
    by PyBullet link index, dropped by hand."""
    path, joints, nj = urdf.path, urdf.joints, len(urdf.joints)
    involved = [int(k) for k in involved_joints]
    A = len(involved)
    if not 1 <= A <= MAX_JOINTS:
        raise InvalidManipulatorFile(f"{path}: {A} involved joints; the chain model holds 1 to {MAX_JOINTS}")
    if len(set(involved)) != A:
        raise InvalidManipulatorFile(f"{path}: involved_joints names a joint twice")
    for what, idxs in (("involved_joints", involved), ("fixed_joints", fixed_joints), ("endeffector_index", [endeffector_index])):
        for k in idxs:
            if not 0 <= int(k) < nj:
                raise InvalidManipulatorFile(f"{path}: {what} names joint index {k}; the file has joints 0 .. {nj - 1}")
    for k in involved:
        if joints[k].type not in _MOVABLE:
            raise InvalidManipulatorFile(f"{path}: involved joint {k} ({joints[k].name!r}) is of type {joints[k].type}: "
                                         "it cannot be driven")
    held = {int(k) for k in fixed_joints} - set(involved)
    init = [float(v) for v in (initial_joint_positions or [])]
    var = [float(v) for v in (initial_positions_variation_range or [])]
    action_of = {k: m for m, k in enumerate(involved)}            # environment.py:466-471: action m drives involved_joints[m]
    joint_of_child = {j.child: k for k, j in enumerate(joints)}

    def constant_value(k: int) -> float:
        """A joint that is not driven: held at 0 (environment.py:474-478), an identity when of fixed type, else parked at its
        initial value (environment.py:284-293 writes entry k to joint index k and nothing moves it afterwards)."""
        if k in held or joints[k].type == "fixed":
            return 0.0
        return init[k] if k < len(init) else 0.0

    def motion(j: UrdfJoint, q: float):
        if j.type == "prismatic":
            return np.eye(3), j.axis * q
        if j.type == "fixed":
            return np.eye(3), np.zeros(3)
        return axis_rotation(j.axis, q), np.zeros(3)

    def path_from_root(link: str) -> List[int]:
        out = []
        while link in joint_of_child:
            k = joint_of_child[link]
            out.append(k)
            link = joints[k].parent
        return out[::-1]

    # the driven joints must form ONE serial chain: each one's nearest driven ancestor is the driven joint before it
    for m, k in enumerate(involved):
        above = [a for a in path_from_root(joints[k].parent) if a in action_of]
        if above != involved[:m]:
            raise InvalidManipulatorFile(
                f"{path}: involved joint {k} ({joints[k].name!r}) does not continue the serial chain of involved_joints "
                f"{involved}: the driven joints above it are {above}, expected {involved[:m]}")

    # pose of every link's frame relative to the frame of the last driven joint above it: (frame, R, t)
    pose = {urdf.root: (0, np.eye(3), np.zeros(3))}
    chain_joints: List[Optional[ChainJoint]] = [None] * A
    reach = 0.0
    for k in sorted(range(nj), key=lambda k: len(path_from_root(joints[k].child))):
        j = joints[k]
        f, R, t = pose[j.parent]
        R, t = _compose(R, t, j.rot, j.xyz)                       # the joint's origin in frame f
        if k in action_of:
            m = action_of[k]
            chain_joints[m] = ChainJoint(
                k, R, t, j.axis, PRISMATIC if j.type == "prismatic" else REVOLUTE, j.limited, j.lower if j.limited else 0.0,
                j.upper if j.limited else 0.0, init[k] if k < len(init) else 0.0, var[k] if k < len(var) else 0.0,
                k if k < A else -1)
            reach += float(np.linalg.norm(t))
            if j.type == "prismatic" and j.limited:
                reach += max(abs(j.lower), abs(j.upper))
            pose[j.child] = (m + 1, np.eye(3), np.zeros(3))
        else:
            Rm, tm = motion(j, constant_value(k))
            R, t = _compose(R, t, Rm, tm)
            pose[j.child] = (f, R, t)

    ee_link = joints[int(endeffector_index)].child
    if not any(a in action_of for a in path_from_root(ee_link)):
        raise InvalidManipulatorFile(f"{path}: the end-effector link (joint index {endeffector_index}) does not descend from the "
                                     f"chain of involved_joints {involved}")
    f_ee, R, t = pose[ee_link]
    inertial = urdf.links[ee_link].inertial_origin                  # getLinkState(...)[0] (environment.py:446): the centre of mass
    ee_point = t + R @ inertial if inertial is not None else t.copy()
    reach += float(np.linalg.norm(ee_point))

    # one capsule per (link, child joint): link frame origin -> the child joint's origin; + the end-effector link's own
    def radius_of(link_name: str) -> float:
        r = urdf.links[link_name].collision_radius
        return float(link_radius) if r is None else float(r)

    segments: List[ChainSegment] = []
    for j in joints:
        f, R, t = pose[j.parent]
        segments.append(ChainSegment(f, t.copy(), t + R @ j.xyz, radius_of(j.parent), joint_of_child.get(j.parent, -1), j.parent))
    segments.append(ChainSegment(f_ee, pose[ee_link][2].copy(), ee_point.copy(), radius_of(ee_link), int(endeffector_index), ee_link))
    segments.sort(key=lambda s: s.frame)                            # (stable: file order within a frame)

    slots = []
    for k in range(A):                                              # environment.py:442-444: slot k <- joint index k
        slots.append((action_of[k], 0.0) if k in action_of else (-1, constant_value(k)))
    model = ChainModel(list(chain_joints), segments, f_ee, ee_point, slots, max(reach, 1e-6), source=os.path.basename(path),
                       initial_positions_variation_range=None if initial_positions_variation_range is None else var)
    if consider_autocollision:
        model.consider_autocollision = True
        _self_pairs(model, urdf, autocollision_ignore)
    planes = ([] if floor_height is None else [(0.0, 0.0, 1.0, floor_height)]) + list(workcell_planes or ())
    if planes or workcell_spheres or workcell_boxes or cell_ignore:
        _workcell(model, urdf, list(workcell_spheres or ()), planes, cell_ignore, list(workcell_boxes or ()))
    return model


def _prune_poses(model: ChainModel) -> np.ndarray:
    """The fixed pose sample [SELF_PRUNE_POSES, A]: uniform inside the limits, +-pi where there are none."""
    rng = np.random.default_rng(SELF_PRUNE_SEED)
    return np.stack([[rng.uniform(j.lower, j.upper) if j.limited else rng.uniform(-math.pi, math.pi) for j in model.joints]
                     for _ in range(SELF_PRUNE_POSES)])


def cell_geometry_name(model: ChainModel, g: int) -> str:
    """'workcell sphere 1 (centre ..., radius ...)' / 'workcell plane 0 (normal ..., offset ...)' / 'workcell box 0 (centre ...,
    half extents ..., radius ...)' of geometry index g."""
    G, H = len(model.cell_spheres), len(model.cell_planes)
    if g >= G + H:
        b = model.cell_boxes[g - G - H]
        return (f"workcell box {g - G - H} (centre {b[0]:.4g} {b[1]:.4g} {b[2]:.4g}, half extents {b[12]:.4g} {b[13]:.4g} {b[14]:.4g}, "
                f"radius {b[15]:.4g})")
    if g < G:
        c = model.cell_spheres[g]
        return f"workcell sphere {g} (centre {c[0]:.4g} {c[1]:.4g} {c[2]:.4g}, radius {c[3]:.4g})"
    n = model.cell_planes[g - G]
    return f"workcell plane {g - G} (normal {n[0]:.4g} {n[1]:.4g} {n[2]:.4g}, offset {n[3]:.4g})"


def _workcell(model: ChainModel, urdf: Urdf, spheres: list, planes: list, ignore: Sequence, boxes: Sequence = ()) -> None:
    """Fills model.cell_spheres / cell_planes / cell_boxes / cell_masks / cell_pairs_dropped: the geometry checked, every pair, the
    hand-made exceptions, then the pruning. A geometry that is left with no tested pair is refused."""
    path, segs = urdf.path, model.segments

    def numbers(v, what, lengths=(4,), said="four finite numbers"):
        try:
            out = tuple(float(x) for x in v)
        except (TypeError, ValueError):
            out = ()
        if len(out) not in lengths or not all(math.isfinite(x) for x in out):
            raise InvalidManipulatorFile(f"{path}: {what} {v!r} is not {said}")
        return out

    def box_record(v):
        """c (3) | R row-major (9) | h (3) | r of an entry of 6, 9 or 10 numbers"""
        b = numbers(v, "workcell box (cx, cy, cz, hx, hy, hz[, roll, pitch, yaw[, r]])", (6, 9, 10), "6, 9 or 10 finite numbers")
        R = rpy_matrix(b[6:9]) if len(b) >= 9 else np.eye(3)
        return b[:3] + tuple(float(x) for x in R.reshape(9)) + b[3:6] + (b[9] if len(b) == 10 else 0.0,)

    model.cell_spheres = [numbers(c, "workcell sphere (cx, cy, cz, r)") for c in spheres]
    model.cell_planes = [numbers(n, "workcell plane (nx, ny, nz, d)") for n in planes]
    model.cell_boxes = [box_record(b) for b in boxes]
    G, n_geom = len(spheres), len(spheres) + len(planes) + len(boxes)
    if n_geom > MAX_CELL:
        raise InvalidManipulatorFile(f"{path}: {n_geom} workcell geometries; a chain model holds at most {MAX_CELL}")
    for k, b in enumerate(model.cell_boxes):
        if min(b[12:15]) < 0.0:
            raise InvalidManipulatorFile(f"{path}: {cell_geometry_name(model, n_geom - len(boxes) + k)} has a negative half extent")
        if b[15] < 0.0:
            raise InvalidManipulatorFile(f"{path}: {cell_geometry_name(model, n_geom - len(boxes) + k)} has a negative radius")
    for g, c in enumerate(model.cell_spheres):
        if c[3] < 0.0:
            raise InvalidManipulatorFile(f"{path}: {cell_geometry_name(model, g)} has a negative radius")
    for h, n in enumerate(model.cell_planes):
        if abs(math.sqrt(n[0] ** 2 + n[1] ** 2 + n[2] ** 2) - 1.0) > 1e-6:
            raise InvalidManipulatorFile(f"{path}: {cell_geometry_name(model, G + h)}: the normal is not a unit vector")
    link_names = {s.link_name for s in segs}
    link_of_index = {s.link: s.link_name for s in segs}
    ignored = set()
    for entry in ignore or ():
        if isinstance(entry, str) or len(entry) != 2:
            raise InvalidManipulatorFile(f"{path}: cell_ignore holds {entry!r}; each entry is (link, geometry index)")
        link, g = entry
        if not isinstance(link, str):
            if isinstance(link, bool) or not isinstance(link, (int, np.integer)) or int(link) not in link_of_index:
                raise InvalidManipulatorFile(f"{path}: cell_ignore names link index {link!r}, which carries no capsule")
            link = link_of_index[int(link)]
        if link not in link_names:
            raise InvalidManipulatorFile(f"{path}: cell_ignore names the link {link!r}, which carries no capsule")
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= int(g) < n_geom:
            raise InvalidManipulatorFile(f"{path}: cell_ignore names workcell geometry {g!r}; the workcell has geometries 0 .. "
                                         f"{n_geom - 1} (spheres first" + (", boxes last" if boxes else "") + ")")
        ignored.add((link, int(g)))
    model.cell_masks = [sum(1 << g for g in range(n_geom) if (s.link_name, g) not in ignored) for s in segs]
    pairs = model.cell_pairs
    if pairs:
        from .kinematic import KinematicEnvironment                 # (the twin imports this module: resolved at call time)
        always = np.all(KinematicEnvironment(model, (0, 0, 0), (0, 0, 0)).cell_clearances(_prune_poses(model)) < 0.0, axis=1)
        for (s, g), drop in zip(pairs, always):
            if drop:
                model.cell_masks[s] &= ~(1 << g)
                if (segs[s].link_name, g) not in model.cell_pairs_dropped:
                    model.cell_pairs_dropped.append((segs[s].link_name, g))
    for g in range(n_geom):
        if not any(mask >> g & 1 for mask in model.cell_masks):
            raise InvalidManipulatorFile(
                f"{path}: {cell_geometry_name(model, g)} is left with no capsule to test: every capsule is in contact with it at "
                f"every one of {SELF_PRUNE_POSES} sampled poses, or dropped by cell_ignore. The geometry cuts through the arm: move it")


def _self_pairs(model: ChainModel, urdf: Urdf, ignore: Sequence) -> None:
    """Fills model.self_pairs / self_pairs_dropped: the reference's pair rule, the hand-made exceptions, then the pruning."""
    path, segs = urdf.path, model.segments
    link_index = {j.child: k for k, j in enumerate(urdf.joints)}

    def index_of(link) -> int:
        if isinstance(link, str):
            if link not in link_index:
                raise InvalidManipulatorFile(f"{path}: autocollision_ignore names the link {link!r}, which is not the child of a "
                                             "joint of the file (the root link takes no part in self-collision)")
            return link_index[link]
        if not 0 <= int(link) < len(urdf.joints):
            raise InvalidManipulatorFile(f"{path}: autocollision_ignore names link index {link}; the file has links 0 .. "
                                         f"{len(urdf.joints) - 1}")
        return int(link)

    ignored = set()
    for pair in ignore or ():
        if isinstance(pair, str) or len(pair) != 2:
            raise InvalidManipulatorFile(f"{path}: autocollision_ignore holds {pair!r}; each entry is a pair of links")
        ignored.add(frozenset(index_of(l) for l in pair))
    # environment.py:394-412 / collision_detector.py:63-98: link i against link j, both in 0 .. num_joints - 1, |i - j| <= 1 left out
    pairs = [(s, t) for s in range(len(segs)) for t in range(s + 1, len(segs))
             if segs[s].link >= 0 and segs[t].link >= 0 and abs(segs[s].link - segs[t].link) > 1
             and frozenset((segs[s].link, segs[t].link)) not in ignored]
    if pairs:
        from .kinematic import KinematicEnvironment                 # (the twin imports this module: resolved at call time)
        q = _prune_poses(model)
        model.self_pairs = pairs
        always = np.all(KinematicEnvironment(model, (0, 0, 0), (0, 0, 0)).pair_clearances(q) < 0.0, axis=1)
        model.self_pairs = [p for p, drop in zip(pairs, always) if not drop]
        model.self_pairs_dropped = [(segs[s].link_name, segs[t].link_name) for (s, t), drop in zip(pairs, always) if drop]
