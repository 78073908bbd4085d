"""Writes tests/golden/chain_ticks_refusals.json: the messages ManipulatorFramework.demonstrate_trajectories refuses its arguments with,
as tests/test_chain_ticks_cpu.py::test_facade_on_the_host_and_its_refusals reads them. Run from the repository root:
    python tests/golden/make_chain_ticks_refusals.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    import chain_traj_common as TC
    from test_chain_ik_cpu import framework
    from test_chain_ticks_cpu import refusals
    f = framework()
    goals = TC.IK.free_poses(f.env.model, f.env, np.random.default_rng(4), 3)
    paths = f.plan_joint_paths(goal_joint_positions=goals, candidates=4, resolution=0.05, seed=2, on_device=False)
    traj = f.plan_trajectories(paths, max_velocity=0.5, max_acceleration=4.0, on_device=False, positions=False)
    with open(os.path.join(HERE, "chain_ticks_refusals.json"), "w") as out:
        json.dump(refusals(f, traj), out, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
