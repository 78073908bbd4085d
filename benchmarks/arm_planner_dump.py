"""Dump what the arm-planning methods of ManipulatorFramework return, array by array, so that two trees can be compared byte for byte:

    python benchmarks/arm_planner_dump.py DIR        on each tree, then cmp the files of the two DIRs

A fixed set of calls on the kinematic iiwa_like7 fixture with scene ranges — 12 queries, candidates=8, resolution=0.05, seed=3, the
shapes of tests/test_chain_cert_gpu.py's framework test: solve_goal_poses, plan_joint_paths (plain, certify=True, roadmap=6, and by
targets=), demonstrate_joint_paths, each with on_device=False (the float64 twin) and, where there is a GPU, with on_device=True; with
a GPU also reach_targets(joint_paths=True) of a freshly seeded agent. Every array field of every result becomes
DIR/<call>.<field>.npy (a device tensor through .cpu()), and DIR/dtypes.txt lists the dtype and shape of each. Every third query's
obstacle sits on the straight line's middle; one more roadmap call takes candidates=1, so that those queries are blocked and
the roadmap has work."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

IIWA_RANGED = dict(manipulator_file=os.path.join(ROOT, "tests", "golden", "urdf", "iiwa_like7.urdf"), endeffector_index=6,
                   fixed_joints=[7], involved_joints=list(range(7)), target_position=[0.45, 0.3, 0.6],
                   obstacle_position=[0.35, 0.2, 0.45], initial_joint_positions=[0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0],
                   initial_positions_variation_range=[0.1, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2], link_radius=0.03,
                   consider_autocollision=True, target_range=[0.15, 0.15, 0.15])
N = 12
KW = dict(candidates=8, resolution=0.05, seed=3)


def fields_of(result):
    """(name, array) of every array a result holds: a named tuple's fields, a dataclass's attributes, JointPaths' roadmap
    attributes, and the members of a nested result under name.member"""
    names = list(getattr(result, "_fields", None) or vars(result))
    names += [n for n in ("nodes", "n_nodes", "roadmap_free_edges") if hasattr(result, n) and n not in names]
    for name in names:
        v = getattr(result, name)
        if torch.is_tensor(v):
            v = v.cpu().numpy()
        if isinstance(v, np.ndarray):
            yield name, v
        elif hasattr(v, "_fields"):
            for sub, a in fields_of(v):
                yield f"{name}.{sub}", a


def queries(env):
    rng = np.random.default_rng(8)
    lo = np.array([j.lower if j.limited else -np.pi for j in env.model.joints])
    hi = np.array([j.upper if j.limited else np.pi for j in env.model.joints])
    start = np.tile(np.asarray(env.initial_joint_positions, float), (N, 1))
    goals = np.clip(start + rng.uniform(-1.2, 1.2, start.shape), lo, hi)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.15, 0.15, (N, 3))
    obstacles = np.tile(env.obstacle_centre if env.scene_ranges_on else env.obstacle_pos, (N, 1)).astype(float)
    obstacles[::3] = env.end_effector(0.5 * (start + goals))[::3]
    return goals, targets, obstacles


def main(out_dir):
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    os.makedirs(out_dir, exist_ok=True)
    out_dir = os.path.abspath(out_dir)
    os.chdir(tempfile.mkdtemp(prefix="arm_planner_dump_"))      # an agent writes its checkpoints where it stands
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(**IIWA_RANGED)
    goals, targets, obstacles = queries(f.env)
    results = {}
    for where, on_device in (("twin", False), ("device", True)):
        if on_device and not torch.cuda.is_available():
            continue
        dev = dict(on_device=on_device)
        results[f"{where}.goal_poses"] = f.solve_goal_poses(targets, obstacles, seed=3, **dev)
        plain = f.plan_joint_paths(goal_joint_positions=goals, obstacles=obstacles, **KW, **dev)
        results[f"{where}.paths"] = plain
        results[f"{where}.paths_certified"] = f.plan_joint_paths(goal_joint_positions=goals, obstacles=obstacles, certify=True, **KW, **dev)
        results[f"{where}.paths_roadmap"] = f.plan_joint_paths(goal_joint_positions=goals, obstacles=obstacles, roadmap=6, **KW, **dev)
        # (with eight candidates a via gets round every obstacle here: the straight line alone leaves queries for the roadmap)
        results[f"{where}.paths_roadmap_straight"] = f.plan_joint_paths(goal_joint_positions=goals, obstacles=obstacles, roadmap=6,
                                                                        **dict(KW, candidates=1), **dev)
        results[f"{where}.paths_to_targets"] = f.plan_joint_paths(targets=targets, obstacles=obstacles, **KW, **dev)
        results[f"{where}.demonstrations"] = f.demonstrate_joint_paths(plain, obstacles=obstacles, frames=200, **dev)
    if torch.cuda.is_available():
        f.set_hyperparameter("batch_size", 64)
        f.set_hyperparameter("buffer_size", 20000)
        np.random.seed(5)
        f.initialize_naf_agent(checkpoint_frequency=64, seed=0)
        results["device.reach"] = f.reach_targets(targets, obstacles, frames=60, joint_paths=True)
    lines = []
    for call, result in results.items():
        for name, a in fields_of(result):
            np.save(os.path.join(out_dir, f"{call}.{name}.npy"), a)
            lines.append(f"{call}.{name} {a.dtype} {list(a.shape)}")
    with open(os.path.join(out_dir, "dtypes.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"{out_dir}: {len(lines)} arrays of {len(results)} calls")


if __name__ == "__main__":
    main(sys.argv[1])
