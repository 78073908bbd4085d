"""Child process of tests/test_chain_scene_gpu.py: `python chain_scene_resume_worker.py <json args>` builds the kinematic
environment of a fixture arm WITH scene ranges (args["arm"] carries target_range / obstacle_range) in a fresh process, resumes
the many-env training from a checkpoint's training_state.pt and writes what the parent compares to args["out"]: scores and
section digests (the learner's, the replay ring's — every stored row carries its episode's scene — and the actor's)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(args):
    from chain_resume_worker import make_framework
    os.chdir(args["cwd"])
    f = make_framework(args["arm"])
    assert f.env.scene_ranges_on
    scores = f.resume_training(args["episode"], args["episodes"], args["frames"], verbose=False, n_envs=args["n_envs"])
    out = {"scores": {str(k): list(v) for k, v in scores.items()},
           "digests": {k: str(v) for k, v in f.naf_agent.training_state_digest().items()}}
    with open(args["out"], "w") as fh:
        json.dump(out, fh)


if __name__ == "__main__":
    main(json.loads(sys.argv[1]))
