"""
Records how ManipulatorFramework's six arm-planning methods refuse a table of bad calls -> tests/golden/arm_planner_refusals.json, on
a machine without a GPU.

Usage:  python tests/golden/make_arm_planner_refusals.py     (writes the JSON of the tree the script stands in)

The committed file was written by this script standing in a checkout of the commit BEFORE arm_planner.py existed (NOTEBOOK.md names
it): the exception class and the full message of every refusal, and — through the rows with two bad arguments at once — which of
them is reported first. tests/test_arm_planner_cpu.py replays every row, and run on a later tree the script must reproduce the file
byte for byte. It therefore goes through the public methods alone.

The environment is the kinematic iiwa_like7 fixture with scene ranges (the one the GPU tests call IIWA_RANGED), "synthetic" the
stand-in environment and "none" no environment; torch.cuda.is_available is False while the rows run, so whatever gets past the
refusals would take the host twin. reach_targets() refuses a missing agent, a data-parallel agent and a bad n_envs before it looks
at its queries. Building an agent needs a GPU, so these rows use a stand-in object that has the one attribute those guards read
(world_size); no row gets as far as the rollout.

Format: one row per call — method, environment ("kinematic" | "synthetic" | "none"), agent ("none" | "single" | "parallel"), kwargs,
raises (class name), message. Values JSON cannot hold are spelled "$nan", "$inf", "$object" (an object()), "$paths" (the JointPaths
of one planned query), "$paths_no_start" (the same without its start poses) and "$paths_3_joints" (poses of three joints).
A bool where a number is expected appears only where the method refuses it: iterations, tolerance, clearance_margin, candidates,
frames of demonstrate_joint_paths and n_envs take True as 1 on both trees, and the pairs that hold one say so by their message.
"""
import contextlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PATH = os.path.join(HERE, "arm_planner_refusals.json")
IIWA_RANGED = dict(manipulator_file=os.path.join(HERE, "urdf", "iiwa_like7.urdf"), endeffector_index=6, fixed_joints=[7],
                   involved_joints=list(range(7)), target_position=[0.45, 0.3, 0.6], obstacle_position=[0.35, 0.2, 0.45],
                   initial_joint_positions=[0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0],
                   initial_positions_variation_range=[0.1, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2], link_radius=0.03,
                   consider_autocollision=True, target_range=[0.15, 0.15, 0.15])
T = [0.45, 0.3, 0.6]                                    # a good target
G = [0.1, 0.7, 0.1, -1.1, 0.1, 0.9, 0.1]                # a good goal pose
FAR = [10.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0]             # joint 0 outside its limits
NUMBER = ["x", "$nan", "$inf", None]                   # what no numeric argument takes


def _rows(method, environment, agent, base, *variants):
    return [dict(method=method, environment=environment, agent=agent, kwargs=dict(base, **v)) for v in variants]


def calls():
    rows = []
    # ---- reach_targets: environment, agent, kinematic, data-parallel, n_envs, the queries (frames first), certify, roadmap, goal_poses
    R = "reach_targets"
    rows += _rows(R, "none", "none", dict(targets=T), {})
    rows += _rows(R, "none", "single", dict(targets=T), {})
    rows += _rows(R, "kinematic", "none", dict(targets=T), {})
    rows += _rows(R, "synthetic", "none", dict(targets=T), {})                       # the agent is missed before the environment's kind
    rows += _rows(R, "synthetic", "single", dict(targets=T), {}, dict(n_envs=0))
    rows += _rows(R, "kinematic", "parallel", dict(targets=T), {}, dict(n_envs=0), dict(targets="abc"))
    rows += _rows(R, "kinematic", "single", dict(targets=T),
                  *[dict(n_envs=v) for v in (0, -1, 1.5, "4")],
                  *[dict(frames=v) for v in (0, -3, True, 1.5, "4", "$nan", None)],
                  *[dict(targets=v) for v in ("abc", [[1.0, 2.0]], [1.0, 2.0, 3.0, 4.0], ["$nan", 0.0, 0.0], [0.0, "$inf", 0.0], [], None)],
                  *[dict(obstacles=v) for v in ("abc", [1.0, 2.0], [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], ["$inf", 0.0, 0.0])],
                  *[dict(initial_joint_positions=v) for v in ("abc", [0.0, 0.0, 0.0], [G, G], FAR, ["$nan"] + G[1:])],
                  *[dict(certify=v) for v in ("yes", 1, None, True)],
                  dict(certify=True, goal_poses=True),
                  *[dict(joint_paths=True, roadmap=v) for v in (63, -1, True, 1.5, "6", None)],
                  dict(joint_paths=True, roadmap=6, certify=True), dict(roadmap=6), dict(roadmap=6, goal_poses=True),
                  dict(goal_poses=True, trajectories=False), dict(joint_paths=True, trajectories=False),
                  # two at once
                  dict(n_envs=0, targets="abc"), dict(n_envs=0, frames=0), dict(n_envs=True, frames=0),
                  dict(frames=0, targets="abc"), dict(targets="abc", obstacles="abc"),
                  dict(obstacles=[1.0, 2.0], initial_joint_positions=FAR), dict(initial_joint_positions=FAR, certify="yes"),
                  dict(targets=[[1.0, 2.0]], certify=True), dict(certify="yes", roadmap=63), dict(certify=True, roadmap=63),
                  dict(joint_paths=True, certify=True, roadmap=63), dict(roadmap=63, goal_poses=True, trajectories=False),
                  dict(roadmap=6, trajectories=False), dict(joint_paths=True, roadmap=6, certify=True, trajectories=False))
    # ---- solve_goal_poses: environment, kinematic, restarts, iterations, tolerance, clearance_margin, seed, the queries
    S = "solve_goal_poses"
    rows += _rows(S, "none", "none", dict(targets=T), {}, dict(restarts=3))
    rows += _rows(S, "synthetic", "none", dict(targets=T), {}, dict(restarts=3))
    rows += _rows(S, "kinematic", "none", dict(targets=T),
                  *[dict(restarts=v) for v in (3, 0, 128, -8, True, 8.0, "8", None)],
                  *[dict(iterations=v) for v in (0, -1, 1.5, "4", None)],
                  *[dict(tolerance=v) for v in (0, 0.0, -1e-3, *NUMBER)],
                  *[dict(clearance_margin=v) for v in NUMBER], dict(clearance_margin="$-inf"),
                  *[dict(seed=v) for v in (-1, True, 1.5, "0", None)],
                  *[dict(targets=v) for v in ("abc", [[1.0, 2.0]], ["$nan", 0.0, 0.0], [])],
                  *[dict(obstacles=v) for v in ([1.0, 2.0], ["$inf", 0.0, 0.0])],
                  *[dict(initial_joint_positions=v) for v in ([0.0, 0.0, 0.0], FAR)],
                  dict(restarts=3, iterations=0), dict(iterations=0, tolerance=0), dict(iterations=True, tolerance=0),
                  dict(tolerance=0, clearance_margin="$nan"), dict(tolerance=True, clearance_margin="$nan"),
                  dict(clearance_margin="$nan", seed=-1), dict(clearance_margin=True, seed=-1), dict(seed=-1, targets="abc"),
                  dict(restarts=3, targets="abc"), dict(targets="abc", initial_joint_positions=FAR))
    # ---- plan_joint_paths: environment, kinematic, one of targets / goals, candidates, resolution, clearance_margin, seed, certify,
    # roadmap, the queries
    P = "plan_joint_paths"
    rows += _rows(P, "none", "none", dict(goal_joint_positions=G), {}, dict(candidates=0))
    rows += _rows(P, "synthetic", "none", dict(goal_joint_positions=G), {}, dict(candidates=0))
    rows += _rows(P, "kinematic", "none", {}, {}, dict(targets=T, goal_joint_positions=G), dict(candidates=0),
                  dict(targets=T, goal_joint_positions=G, candidates=0))
    rows += _rows(P, "kinematic", "none", dict(goal_joint_positions=G),
                  *[dict(candidates=v) for v in (0, 65, -1, 1.5, "8", None)],
                  *[dict(resolution=v) for v in (0, 0.0, -0.1, True, *NUMBER)],
                  *[dict(clearance_margin=v) for v in NUMBER],
                  *[dict(seed=v) for v in (-1, True, 1.5, "0", None)],
                  *[dict(certify=v) for v in ("yes", 1, 0, None)],
                  *[dict(roadmap=v) for v in (63, -1, True, 1.5, "6", None)], dict(roadmap=6, certify=True),
                  *[dict(goal_joint_positions=v) for v in ("abc", [0.0, 0.0, 0.0], [[0.0, 0.0, 0.0]], [G[:6]], FAR, [G, FAR],
                                                           ["$nan"] + G[1:], [], "$object")],
                  *[dict(obstacles=v) for v in ([1.0, 2.0], ["$inf", 0.0, 0.0], [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])],
                  *[dict(initial_joint_positions=v) for v in ([0.0, 0.0, 0.0], FAR, [G, G])],
                  dict(candidates=0, resolution=0), dict(candidates=True, resolution=0), dict(resolution=0, clearance_margin="$nan"),
                  dict(clearance_margin="$nan", seed=-1), dict(clearance_margin=True, seed=-1), dict(seed=-1, certify="yes"),
                  dict(certify="yes", roadmap=63), dict(certify=True, roadmap=63), dict(roadmap=63, goal_joint_positions="abc"),
                  dict(roadmap=6, certify=True, goal_joint_positions="abc"), dict(goal_joint_positions=FAR, initial_joint_positions=FAR),
                  dict(goal_joint_positions="abc", obstacles=[1.0, 2.0]), dict(obstacles=[1.0, 2.0], initial_joint_positions=FAR))
    rows += _rows(P, "kinematic", "none", dict(targets=T),
                  *[dict(targets=v) for v in ("abc", [[1.0, 2.0]], ["$nan", 0.0, 0.0])],
                  dict(obstacles=[1.0, 2.0]), dict(initial_joint_positions=FAR), dict(targets="abc", seed=-1),
                  dict(targets="abc", obstacles=[1.0, 2.0]))
    # ---- demonstrate_joint_paths: environment, kinematic, paths, speed, frames, the number of joints, targets and obstacles
    D = "demonstrate_joint_paths"
    rows += _rows(D, "none", "none", dict(paths="$paths"), {}, dict(paths=None))
    rows += _rows(D, "synthetic", "none", dict(paths="$paths"), {}, dict(paths=None))
    rows += _rows(D, "kinematic", "none", dict(paths="$paths"),
                  *[dict(paths=v) for v in (None, "x", "$object", "$paths_no_start", "$paths_3_joints")],
                  *[dict(speed=v) for v in (0, 0.0, -1, 1.5, True, *NUMBER)],
                  *[dict(frames=v) for v in (0, 1025, -1, 1.5, "4", None)],
                  *[dict(targets=v) for v in ("abc", [[1.0, 2.0]], [T, T], ["$nan", 0.0, 0.0])],
                  *[dict(obstacles=v) for v in ([1.0, 2.0], ["$inf", 0.0, 0.0], [T, T])],
                  dict(paths=None, speed=0), dict(paths="$paths_no_start", frames=0), dict(speed=0, frames=0),
                  dict(speed=0, paths="$paths_3_joints"), dict(frames=0, paths="$paths_3_joints"), dict(frames=True, speed=2),
                  dict(paths="$paths_3_joints", targets="abc"), dict(targets="abc", obstacles=[1.0, 2.0]),
                  dict(targets=[T, T], obstacles=[1.0, 2.0]))
    return rows


def decode(v, special):
    if isinstance(v, str) and v.startswith("$"):
        return special[v]() if callable(special[v]) else special[v]
    if isinstance(v, list):
        return [decode(x, special) for x in v]
    return v


@contextlib.contextmanager
def no_gpu():
    real = torch.cuda.is_available
    torch.cuda.is_available = lambda: False
    try:
        yield
    finally:
        torch.cuda.is_available = real


class Replay:
    """The frameworks the rows run on, built once: replay(row) -> (class name, message) of what the call raises."""

    def __init__(self):
        from robotic_manipulator_rloa_amd import ManipulatorFramework
        self.frameworks = {"none": ManipulatorFramework(), "synthetic": ManipulatorFramework(), "kinematic": ManipulatorFramework()}
        self.frameworks["synthetic"].initialize_synthetic_environment()
        self.frameworks["kinematic"].initialize_kinematic_environment(**IIWA_RANGED)
        self.agents = {"none": None, "single": types.SimpleNamespace(world_size=1), "parallel": types.SimpleNamespace(world_size=2)}
        with no_gpu():
            paths = self.frameworks["kinematic"].plan_joint_paths(goal_joint_positions=G, candidates=1, resolution=1.0)
        cut = lambda a: np.asarray(a)[:, :3]      # noqa: E731
        self.special = {"$nan": float("nan"), "$inf": float("inf"), "$-inf": float("-inf"), "$object": object, "$paths": paths,
                        "$paths_no_start": paths._replace(start=None),
                        "$paths_3_joints": paths._replace(start=cut(paths.start), goal=cut(paths.goal), via=cut(paths.via))}

    def __call__(self, row):
        f = self.frameworks[row["environment"]]
        f.naf_agent = self.agents[row["agent"]]
        kwargs = {k: decode(v, self.special) for k, v in row["kwargs"].items()}
        try:
            with no_gpu():
                getattr(f, row["method"])(**kwargs)
        except Exception as e:      # noqa: BLE001 — the class is what is recorded
            return type(e).__name__, str(e)
        finally:
            f.naf_agent = None
        raise AssertionError(f"not refused: {row}")


def record():
    replay = Replay()
    out = []
    for row in calls():
        name, message = replay(row)
        out.append(dict(row, raises=name, message=message))
    return out


def render(rows) -> str:
    return "[\n" + ",\n".join(json.dumps(r, allow_nan=False) for r in rows) + "\n]\n"


def main():
    rows = record()
    with open(PATH, "w") as f:
        f.write(render(rows))
    kinds = sorted({r["raises"] for r in rows})
    print(f"{PATH}: {len(rows)} refusals ({', '.join(kinds)}), {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
