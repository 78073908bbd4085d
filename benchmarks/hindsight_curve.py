"""What hindsight goals do to learning, at equal env-steps: the README's example arm (tests/golden/urdf/iiwa_like7.urdf, target
box of half-widths 0.15 / 0.15 / 0.1) trained with hindsight 0, 0.5 and 0.8, three seeds each, then scored by the share of 2000
fixed reach_targets queries from the target box that end 'reached' (deterministic policy, 400 frames).

  python benchmarks/hindsight_curve.py --vector-steps 3000 --out profiles/hindsight_curve.json

Every run takes `--vector-steps` vector steps of `--envs` envs (env-steps = their product) with one update per env-step, as
run_training does. The JSON holds every run's score, outcome counts, hindsight shares of its last chunk and seconds, and per ratio
the mean and the spread over the seeds. The queries are the same for every run (seed 12345)."""
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


def one_run(ratio, seed, a, targets):
    import numpy as np
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    np.random.seed(seed)
    f = ManipulatorFramework()
    f.set_hyperparameter("batch_size", a.batch)
    f.initialize_kinematic_environment(**ARM)
    f.initialize_naf_agent(checkpoint_frequency=10 ** 9, seed=seed)
    stats = f.naf_agent.run_vectorized(a.vector_steps, n_envs=a.envs, max_frames=a.frames, hindsight=ratio,
                                       hindsight_horizon=a.horizon, **f._device_env_arguments())
    plan = f.reach_targets(targets, frames=a.frames, trajectories=False)
    names, counts = np.unique(plan.outcome, return_counts=True)
    out = {"hindsight": ratio, "seed": seed, "reached_share": float(np.mean(plan.outcome == "reached")),
           "outcomes": {str(n): int(c) for n, c in zip(names, counts)}, "mean_final_distance": float(np.mean(plan.final_distance)),
           "env_steps": stats["env_steps"], "updates": stats["updates"], "seconds": round(stats["seconds"], 2),
           "episodes_finished": stats["episodes_finished"]}
    out.update({k: round(v, 4) for k, v in stats.items() if k.startswith("hindsight")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vector-steps", type=int, default=3000)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--horizon", type=int, default=None, help="hindsight_horizon (default: --frames)")
    ap.add_argument("--ratios", type=float, nargs="+", default=[0.0, 0.5, 0.8])
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hindsight_curve.json"))
    a = ap.parse_args()
    import numpy as np
    out_path = os.path.abspath(a.out)
    os.chdir(tempfile.mkdtemp())          # model.p and logs of the runs
    rng = np.random.default_rng(12345)
    targets = np.array(ARM["target_position"]) + rng.uniform(-1.0, 1.0, (a.queries, 3)) * np.array(ARM["target_range"])
    runs = []
    for ratio in a.ratios:
        for seed in a.seeds:
            runs.append(one_run(ratio, seed, a, targets))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for ratio in a.ratios:
        s = [r["reached_share"] for r in runs if r["hindsight"] == ratio]
        summary[str(ratio)] = {"mean": float(np.mean(s)), "min": float(np.min(s)), "max": float(np.max(s))}
    result = {"arm": "iiwa_like7", "target_range": ARM["target_range"], "envs": a.envs, "batch": a.batch, "frames": a.frames,
              "vector_steps": a.vector_steps, "env_steps": a.vector_steps * a.envs, "queries": a.queries, "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"summary": summary, "out": out_path}))


if __name__ == "__main__":
    main()
