"""Child process of tests/test_hindsight_gpu.py: `python hindsight_resume_worker.py <json args>` builds the kinematic environment
of a fixture arm in a fresh process, resumes the many-env training WITH hindsight goals (args["hindsight"]) from a checkpoint's
training_state.pt and writes what the parent compares to args["out"]: scores and section digests (the replay ring's rows carry
their episode tags, the sampler's counter places the hindsight draws)."""
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
    scores = f.resume_training(args["episode"], args["episodes"], args["frames"], verbose=False, n_envs=args["n_envs"],
                               hindsight=args["hindsight"])
    assert "hindsight_relabelled_share" in f.naf_agent.last_run_stats
    out = {"scores": {str(k): list(v) for k, v in scores.items()},
           "digests": {k: str(v) for k, v in f.naf_agent.training_state_digest().items()}}
    with open(args["out"], "w") as fh:
        json.dump(out, fh)


if __name__ == "__main__":
    main(json.loads(sys.argv[1]))
