"""Resume from a saved full training state (robotic_manipulator_rloa_amd/training_state.py): a resumed run is the same run as
the uninterrupted one — scores, weights, every section of the state and every action, compared exactly."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from resume_worker import DEV, HashEnv, make_agent, model_file

pytestmark = pytest.mark.gpu
F, N = 80, 8                       # frames per episode, episodes; checkpoints every 2 episodes


def _in(d):
    os.makedirs(d, exist_ok=True)
    os.chdir(d)


def _assert_model_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _run_full(root, **kw):
    _in(os.path.join(root, "full"))
    env = HashEnv()
    agent = make_agent(env, **kw)
    scores = agent.run(F, N, False)
    return scores, env.hashes, agent.training_state_digest(), model_file()


@pytest.mark.parametrize("B,uf,nu,p_mode", [(64, 1, 1, "hadamard"), (256, 1, 1, "hadamard"), (64, 2, 3, "hadamard"),
                                            (64, 1, 1, "matmul")])
def test_run_resumed_from_a_checkpoint_is_the_uninterrupted_run(tmp_path, B, uf, nu, p_mode):
    kw = dict(B=B, update_freq=uf, num_updates=nu, p_mode=p_mode)
    root = str(tmp_path)
    try:
        scores, hashes, digests, model = _run_full(root, **kw)
        assert digests["learner"] and len(hashes) > B           # (the gate opened: the learner has been trained)
        # the first half, saving, then a fresh agent that loads the half-way checkpoint
        _in(os.path.join(root, "split"))
        env1 = HashEnv()
        a1 = make_agent(env1, save=True, **kw)
        a1.run(F, N // 2, False)
        ck = f"checkpoints/{N // 2}/training_state.pt"
        assert os.path.isfile(ck) and os.path.isfile("checkpoints/2/training_state.pt")
        if B == 64:                                             # (the state saved half-way has been trained)
            assert torch.load(ck, weights_only=True)["sections"]["learner"]["tensors"]["step_dev"].item() > 0
        env2 = HashEnv()
        a2 = make_agent(env2, **kw)
        a2.load_training_state(ck)
        got = a2.run(F, N, False, resume=True)
        assert got == scores
        assert env1.hashes + env2.hashes == hashes
        assert a2.training_state_digest() == digests
        _assert_model_equal(model_file(), model)
        if (B, uf, nu, p_mode) != (64, 1, 1, "hadamard"):
            return
        # once more in a fresh process: nothing the result depends on lives in the process that saved
        _in(os.path.join(root, "child"))
        shutil.copyfile(os.path.join(root, "split", ck), "state.pt")
        args = dict(cwd=os.getcwd(), state="state.pt", out="out.json", B=B, update_freq=uf, num_updates=nu, p_mode=p_mode,
                    frames=F, episodes=N)
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "resume_worker.py"),
                            json.dumps(args)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        out = json.load(open("out.json"))
        assert {int(k): tuple(v) for k, v in out["scores"].items()} == scores
        assert env1.hashes + out["hashes"] == hashes
        assert {k: int(v) for k, v in out["digests"].items()} == digests
        _assert_model_equal({k: np.asarray(v, np.float32) for k, v in out["model"].items()}, model)
    finally:
        os.chdir(root)


def test_saving_does_not_perturb_the_run(tmp_path):
    root = str(tmp_path)
    try:
        scores, hashes, digests, model = _run_full(root)
        _in(os.path.join(root, "saving"))
        env = HashEnv()
        agent = make_agent(env, save=True)
        assert agent.run(F, N, False) == scores
        assert env.hashes == hashes and agent.training_state_digest() == digests
        _assert_model_equal(model_file(), model)
        assert all(os.path.isfile(f"checkpoints/{e}/training_state.pt") for e in range(2, N + 1, 2))
    finally:
        os.chdir(root)


def _drive(agent, data, lo, hi):
    """act / step over transitions [lo, hi) of a scripted stream; actions as returned"""
    st, _, rw, ns, dn = data
    out = []
    for t in range(lo, hi):
        a = agent.act(st[t])
        out.append(np.array(a, np.float32, copy=True))
        agent.step(st[t], a, float(rw[t]), ns[t], int(dn[t]))
    return out


def _stream(n, S, A, seed=3):
    """transitions in which state t + 1 is next_state t (the loop asks act() about the state the last step() named)"""
    from synth_data import make_transitions
    st, ac, rw, ns, dn = make_transitions(n, S, A, seed=seed, rare_events=False)
    st[1:] = ns[:-1]
    return st, ac, rw, ns, dn


@pytest.mark.parametrize("S,A,B", [(21, 6, 64), (33, 12, 64)])
def test_mid_episode_save_gives_every_later_action(tmp_path, S, A, B):
    """A save between step() and the next act(): where the graph's tail has drawn the next action already (the fused path,
    (21, 6)), the resumed agent's first act() returns that action; the unfused chain (33, 12) has no tail."""
    import warnings
    os.chdir(tmp_path)
    n, cut = B + 120, B + 47
    data = _stream(n, S, A)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = make_agent(object(), B=B, S=S, A=A)
        acts = _drive(full, data, 0, n)
        d_full = full.training_state_digest()
        half = make_agent(object(), B=B, S=S, A=A)
        first = _drive(half, data, 0, cut)
        if A == 6:
            assert half._ahead is not None                              # (the case this test is for)
        half.save_training_state("mid.pt")
        rest = make_agent(object(), B=B, S=S, A=A)
        rest.load_training_state("mid.pt")
        second = _drive(rest, data, cut, n)
    assert len(first + second) == len(acts)
    for t, (x, y) in enumerate(zip(first + second, acts)):
        np.testing.assert_array_equal(x, y, err_msg=f"action {t}")
    assert rest.training_state_digest() == d_full
    assert rest.last_loss() == full.last_loss()


def test_restore_into_an_agent_that_has_trained(tmp_path):
    """The restore writes in place into an agent whose graphs are captured and whose pipeline is armed: its next timestep
    starts over from the restored public state, and the continuation is the uninterrupted one."""
    os.chdir(tmp_path)
    B, n, cut = 64, 220, 150
    data = _stream(n, 21, 6)
    full = make_agent(object(), B=B)
    acts = _drive(full, data, 0, n)
    half = make_agent(object(), B=B)
    first = _drive(half, data, 0, cut)
    half.save_training_state("mid.pt")
    other = make_agent(object(), B=B)
    _drive(other, _stream(n, 21, 6, seed=11), 0, B + 90)       # its own run: graphs, pipeline, another ring
    pipe = other._chunk.pipe
    slow0 = pipe.slow_runs if pipe is not None else 0
    other.load_training_state("mid.pt")
    second = _drive(other, data, cut, n)
    if pipe is not None:
        assert pipe.slow_runs >= slow0 + 1                      # started over from the restored public state
    for t, (x, y) in enumerate(zip(first + second, acts)):
        np.testing.assert_array_equal(x, y, err_msg=f"action {t}")
    assert other.training_state_digest() == full.training_state_digest()


def test_restore_before_the_gate_into_an_agent_that_has_trained(tmp_path):
    """A state saved before learning started (len(memory) <= batch_size), restored into an agent whose gate is open and whose
    step() takes its short way: the gate closes again, and the continuation is the uninterrupted one."""
    os.chdir(tmp_path)
    B, n, cut = 64, 200, 40
    data = _stream(n, 21, 6)
    full = make_agent(object(), B=B)
    acts = _drive(full, data, 0, n)
    half = make_agent(object(), B=B)
    first = _drive(half, data, 0, cut)
    assert int(half.learner.step_dev.item()) == 0             # (nothing learned yet)
    half.save_training_state("early.pt")
    other = make_agent(object(), B=B)
    _drive(other, _stream(n, 21, 6, seed=11), 0, B + 90)
    assert other._fast is not None and int(other.learner.step_dev.item()) > 0
    other.load_training_state("early.pt")
    second = _drive(other, data, cut, B)                      # B rows in the ring: the gate is still closed, no update
    assert int(other.learner.step_dev.item()) == 0
    second += _drive(other, data, B, n)
    for t, (x, y) in enumerate(zip(first + second, acts)):
        np.testing.assert_array_equal(x, y, err_msg=f"action {t}")
    assert other.training_state_digest() == full.training_state_digest()


def test_step_without_act_after_a_restore_draws_its_own_next_action(tmp_path):
    """load, then step() with the action the saved run took (no act()), then save: the file holds the action this step()'s
    graph drew, not the one restored, and a third agent continues as the uninterrupted run."""
    os.chdir(tmp_path)
    B, n, cut = 64, 200, 130
    data = _stream(n, 21, 6)
    st, _, rw, ns, dn = data
    full = make_agent(object(), B=B)
    acts = _drive(full, data, 0, n)
    half = make_agent(object(), B=B)
    _drive(half, data, 0, cut)
    half.save_training_state("a.pt")
    mid = make_agent(object(), B=B)
    mid.load_training_state("a.pt")
    mid.step(st[cut], acts[cut], float(rw[cut]), ns[cut], int(dn[cut]))
    mid.save_training_state("b.pt")
    last = make_agent(object(), B=B)
    last.load_training_state("b.pt")
    rest = _drive(last, data, cut + 1, n)
    for t, (x, y) in enumerate(zip(rest, acts[cut + 1:])):
        np.testing.assert_array_equal(x, y, err_msg=f"action {cut + 1 + t}")
    assert last.training_state_digest() == full.training_state_digest()


def _vec(agent, episodes, resume=False):
    return agent.run_vectorized(n_envs=64, max_frames=16, episodes=episodes, drain_every=8, resume=resume)


def test_run_vectorized_resumes_and_extends(tmp_path):
    root = str(tmp_path)
    kw = dict(checkpoint_frequency=64)
    try:
        _in(os.path.join(root, "full"))
        full = make_agent(None, save=True, **kw)
        r_full = _vec(full, 256)
        d_full = full.training_state_digest()
        assert r_full["checkpoints"] == [64, 128, 192, 256]
        # from a checkpoint that is not the last one
        again = make_agent(None, **kw)
        again.load_training_state("checkpoints/128/training_state.pt")
        r = _vec(again, 256, resume=True)
        assert r["scores"] == r_full["scores"] and again.training_state_digest() == d_full
        # extended: the last checkpoint to twice the budget, against an uninterrupted run of that budget
        _in(os.path.join(root, "long"))
        long = make_agent(None, **kw)
        r_long = _vec(long, 512)
        ext = make_agent(None, **kw)
        ext.load_training_state(os.path.join(root, "full", "checkpoints/256/training_state.pt"))
        r_ext = _vec(ext, 512, resume=True)
        assert r_ext["scores"] == r_long["scores"] and r_ext["checkpoints"] == r_long["checkpoints"]
        assert ext.training_state_digest() == long.training_state_digest()
        # a different loop is refused
        other = make_agent(None, **kw)
        other.load_training_state(os.path.join(root, "full", "checkpoints/128/training_state.pt"))
        with pytest.raises(ValueError, match="max_frames"):
            other.run_vectorized(n_envs=64, max_frames=20, episodes=256, drain_every=8, resume=True)
    finally:
        os.chdir(root)


def test_refusals(tmp_path):
    from robotic_manipulator_rloa_amd import _lib
    os.chdir(tmp_path)
    data = _stream(120, 21, 6)
    agent = make_agent(object())
    _drive(agent, data, 0, 100)
    agent.save_training_state("ok.pt")
    st = torch.load("ok.pt", weights_only=True)
    rows = st["sections"]["replay"]["tensors"]["rows"]
    rows.view(-1).view(torch.uint8)[12345] ^= 0x10                      # one flipped byte in the ring
    torch.save(st, "bad.pt")
    fresh = make_agent(object())
    d0 = fresh.training_state_digest()
    with pytest.raises(ValueError, match="'replay'"):
        fresh.load_training_state("bad.pt")
    assert fresh.training_state_digest() == d0                 # nothing was committed
    with pytest.raises(ValueError, match="learning_rate"):
        make_agent(object(), lr=2e-3).load_training_state("ok.pt")
    with pytest.raises(ValueError, match="batch_size"):
        make_agent(object(), B=128).load_training_state("ok.pt")
    fresh.load_training_state("ok.pt")                         # (the good file loads)
    assert fresh.training_state_digest() == agent.training_state_digest()
    with pytest.raises(ValueError, match="run_vectorized"):
        fresh.run_vectorized(n_envs=64, max_frames=16, episodes=8, resume=True)    # a file saved outside a loop
    agent.world_size = 2                                       # (what a data-parallel agent says of itself)
    with pytest.raises(_lib.NafHipError, match="data parallel"):
        agent.save_training_state("dp.pt")
    saving = make_agent(object(), save=True)
    with pytest.raises(_lib.NafHipError, match="worker processes"):
        saving.run_host_vectorized(None, vector_steps=1)
    with pytest.raises(_lib.NafHipError, match="worker processes"):
        fresh.run_host_vectorized(None, vector_steps=1, resume=True)


def _twin(words, start=0):
    """numpy twin of naf_state_digest (csrc/state_digest.hip), over words [start, start + len)"""
    w = np.asarray(words, np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = (np.arange(w.size, dtype=np.uint64) + np.uint64(start)) * np.uint64(0x9E3779B97F4A7C15) + w
        x = (x ^ (x >> np.uint64(32))) * np.uint64(0xD6E8FEB86659FD93)
        x ^= x >> np.uint64(32)
        return int(x.sum(dtype=np.uint64))


def test_state_digest_kernel_against_its_numpy_twin():
    from robotic_manipulator_rloa_amd.training_state import device_digests
    rng = np.random.default_rng(7)
    sizes = [0, 1, 3, 4095, 4096, 1000007]
    host = [rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for n in sizes]
    dev = [torch.from_numpy(h.view(np.int32)).to(DEV) for h in host]
    want = [_twin(h) for h in host]
    assert want[0] == 0
    for blocks in (0, 1, 7, 300, 4096):
        assert device_digests(dev, blocks) == want, blocks
    # a segment that does not start on 16 bytes, and more segments than one launch takes
    big = torch.from_numpy(host[-1].view(np.int32)).to(DEV)
    assert device_digests([big[1:], big[3:4098]]) == [_twin(host[-1][1:]), _twin(host[-1][3:4098])]
    many = [torch.from_numpy(rng.integers(0, 2 ** 32, 1 + 37 * i, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(DEV)
            for i in range(45)]
    assert device_digests(many) == [_twin(t.cpu().numpy()) for t in many]
    # any single flipped word changes it
    for pos in (0, 1, 4095, 500000, 1000006):
        for bit in (0, 17, 31):
            flipped = big.clone()
            flipped[pos] ^= (1 << bit) if bit < 31 else -(1 << 31)
            assert device_digests([flipped])[0] != want[-1], (pos, bit)
