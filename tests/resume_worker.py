"""Helpers of tests/test_resume_gpu.py, and its child process: `python resume_worker.py <json args>` loads a training state
into a fresh agent in a fresh process, finishes the run and writes what the parent compares (scores, model.p's tensors as
lists, section digests, the hashes of the actions taken) to args["out"]."""
import hashlib
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = torch.device("cuda:0")


class HashEnv:
    """SyntheticEnvironment(n) that keeps a hash of every action it is given."""

    def __init__(self, n=6):
        from robotic_manipulator_rloa_amd.environment.synthetic import SyntheticEnvironment
        self.env = SyntheticEnvironment(n)
        self.observation_space, self.action_space = self.env.observation_space, self.env.action_space
        self.hashes = []

    def reset(self, verbose=True):
        return self.env.reset(verbose)

    def step(self, action):
        self.hashes.append(hashlib.sha1(np.ascontiguousarray(action, np.float32).tobytes()).hexdigest())
        return self.env.step(action)


def make_agent(env, B=64, update_freq=1, num_updates=1, p_mode="hadamard", save=False, S=21, A=6, buffer_size=10000,
               checkpoint_frequency=2, lr=1e-3):
    from robotic_manipulator_rloa_amd.naf_components.naf_algorithm import NAFAgent
    np.random.seed(5)                    # (the agent seeds `random` and torch; numpy's global generator is the caller's)
    return NAFAgent(env, S, A, 256, B, buffer_size, lr, 1e-3, 0.99, update_freq, num_updates, checkpoint_frequency, DEV, 0,
                    p_mode=p_mode, save_training_state=save)


def model_file(path="model.p"):
    return {k: v.numpy() for k, v in torch.load(path, map_location="cpu", weights_only=True).items()}


def main(args):
    os.chdir(args["cwd"])
    env = HashEnv()
    agent = make_agent(env, args["B"], args["update_freq"], args["num_updates"], args["p_mode"])
    agent.load_training_state(args["state"])
    scores = agent.run(args["frames"], args["episodes"], False, resume=True)
    out = {"scores": {str(k): list(v) for k, v in scores.items()}, "hashes": env.hashes,
           "digests": {k: str(v) for k, v in agent.training_state_digest().items()},
           "model": {k: v.tolist() for k, v in model_file().items()}}
    with open(args["out"], "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(json.loads(sys.argv[1]))
