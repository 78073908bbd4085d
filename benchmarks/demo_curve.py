"""What planned joint paths as demonstrations do to learning, at equal env-steps: the README's example arm
(tests/golden/urdf/iiwa_like7.urdf, target box of half-widths 0.15 / 0.15 / 0.1) trained without and with demonstrations in the
replay ring, three seeds each, then scored by the share of 2000 fixed reach_targets queries from the target box that end 'reached'
(deterministic policy, 400 frames).

  python benchmarks/demo_curve.py --vector-steps 3000 --out profiles/demo_curve.json

The demonstrations are made once per seed before the run: `--demos` targets drawn from the target box (seed 777 + seed, not the
queries'), plan_joint_paths from the initial pose, demonstrate_joint_paths at `--speed`, and the kept rows appended to the ring
before the first tick (run_vectorized(demonstrations=)). Every run takes `--vector-steps` vector steps of `--envs` envs (env-steps
= their product; the demonstration rows are NOT counted as env-steps) with one update per env-step, as run_training does. The JSON
holds every run's score, outcome counts, demonstration counts and seconds, and per arm of the comparison the mean and the spread
over the seeds. The queries are the same for every run (seed 12345)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARM = dict(manipulator_file=os.path.join(ROOT, "tests", "golden", "urdf", "iiwa_like7.urdf"), endeffector_index=6, fixed_joints=[7],
           involved_joints=[0, 1, 2, 3, 4, 5, 6], target_position=[0.45, 0.3, 0.6], obstacle_position=[0.35, 0.2, 0.45],
           initial_joint_positions=[0, 0.6, 0, -1.2, 0, 0.8, 0], link_radius=0.03, target_range=[0.15, 0.15, 0.1])


def one_run(with_demos, seed, a, targets):
    import numpy as np
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    np.random.seed(seed)
    f = ManipulatorFramework()
    f.set_hyperparameter("batch_size", a.batch)
    f.initialize_kinematic_environment(**ARM)
    f.initialize_naf_agent(checkpoint_frequency=10 ** 9, seed=seed)
    demos = None
    if with_demos:
        rng = np.random.default_rng(777 + seed)
        shown = np.array(ARM["target_position"]) + rng.uniform(-1.0, 1.0, (a.demos, 3)) * np.array(ARM["target_range"])
        demos = f.demonstrate_joint_paths(f.plan_joint_paths(shown, seed=seed), speed=a.speed, frames=a.frames)
    stats = f.naf_agent.run_vectorized(a.vector_steps, n_envs=a.envs, max_frames=a.frames, demonstrations=demos,
                                       **f._device_env_arguments())
    plan = f.reach_targets(targets, frames=a.frames, trajectories=False)
    names, counts = np.unique(plan.outcome, return_counts=True)
    out = {"demonstrations": bool(with_demos), "seed": seed, "reached_share": float(np.mean(plan.outcome == "reached")),
           "outcomes": {str(n): int(c) for n, c in zip(names, counts)}, "mean_final_distance": float(np.mean(plan.final_distance)),
           "env_steps": stats["env_steps"], "updates": stats["updates"], "seconds": round(stats["seconds"], 2),
           "episodes_finished": stats["episodes_finished"]}
    out.update({k: int(v) for k, v in stats.items() if k.startswith("demonstration")})
    if demos is not None:
        names, counts = np.unique(demos.outcome, return_counts=True)
        out["demonstration_outcomes"] = {str(n): int(c) for n, c in zip(names, counts)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vector-steps", type=int, default=3000)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--demos", type=int, default=256, help="targets shown as demonstrations per run")
    ap.add_argument("--speed", type=float, default=1.0)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demo_curve.json"))
    a = ap.parse_args()
    import numpy as np
    out_path = os.path.abspath(a.out)
    os.chdir(tempfile.mkdtemp())          # model.p and logs of the runs
    rng = np.random.default_rng(12345)
    targets = np.array(ARM["target_position"]) + rng.uniform(-1.0, 1.0, (a.queries, 3)) * np.array(ARM["target_range"])
    runs = []
    for with_demos in (False, True):
        for seed in a.seeds:
            runs.append(one_run(with_demos, seed, a, targets))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for with_demos in (False, True):
        s = [r["reached_share"] for r in runs if r["demonstrations"] == with_demos]
        summary["with" if with_demos else "without"] = {"mean": float(np.mean(s)), "min": float(np.min(s)), "max": float(np.max(s))}
    result = {"arm": "iiwa_like7", "target_range": ARM["target_range"], "envs": a.envs, "batch": a.batch, "frames": a.frames,
              "vector_steps": a.vector_steps, "env_steps": a.vector_steps * a.envs, "queries": a.queries, "demos": a.demos,
              "speed": a.speed, "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"summary": summary, "out": out_path}))


if __name__ == "__main__":
    main()
