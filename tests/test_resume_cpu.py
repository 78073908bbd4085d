"""The parts of resuming from a saved training state that need no GPU: the digest's numpy twin, the file checks and their
messages, the loop-position checks and ManipulatorFramework.resume_training's arguments."""
import os

import numpy as np
import pytest
import torch

from robotic_manipulator_rloa_amd import training_state as ts


def _twin(words, start=0):
    """naf_state_digest (csrc/state_digest.hip) over words [start, start + len): sum of mix(i, w_i) mod 2^64"""
    w = np.asarray(words, np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = (np.arange(w.size, dtype=np.uint64) + np.uint64(start)) * np.uint64(0x9E3779B97F4A7C15) + w
        x = (x ^ (x >> np.uint64(32))) * np.uint64(0xD6E8FEB86659FD93)
        x ^= x >> np.uint64(32)
        return int(x.sum(dtype=np.uint64))


def test_digest_twin_properties():
    rng = np.random.default_rng(1)
    w = rng.integers(0, 2 ** 32, 100003, dtype=np.uint64).astype(np.uint32)
    d = _twin(w)
    assert d == ts.digest_words_np(w) and _twin(w[:0]) == 0 and 0 <= d < 2 ** 64
    # any split into pieces adds up to the whole: the digest does not depend on how a grid divides the words
    for cuts in ([0, 1, 4096, 100003], [0, 3, 50000, 77777, 100003]):
        assert sum(_twin(w[a:b], a) for a, b in zip(cuts, cuts[1:])) % 2 ** 64 == d
    # a changed word always changes it; so does a swap of two different words
    for pos in (0, 1, 99999, 100002):
        for delta in (1, 1 << 31, 0xFFFFFFFF):
            v = w.copy()
            v[pos] ^= np.uint32(delta)
            assert _twin(v) != d
    v = w.copy()
    v[[10, 20]] = v[[20, 10]]
    assert w[10] != w[20] and _twin(v) != d
    # the same words of another length are another digest; zeros count by their position
    assert _twin(np.zeros(5, np.uint32)) != _twin(np.zeros(6, np.uint32))
    assert ts.digest_bytes(b"abc") == _twin(np.frombuffer(b"abc\0", np.uint32))


def _state_file(path, **changes):
    cfg = {"state_size": 21, "action_size": 6, "layer_size": 256, "batch_size": 64, "buffer_size": 1000, "learning_rate": 1e-3,
           "tau": 1e-3, "gamma": 0.99, "update_freq": 1, "num_updates": 1, "p_mode": 0, "action_mode": 0, "seed": 0}
    secs = {s: {"tensors": {}, "meta": {}} for s in ts.SECTIONS}
    st = {"format": ts.FORMAT, "version": ts.VERSION, "abi": ts._lib.header_abi_version(), "config": cfg, "sections": secs,
          "digests": {s: 0 for s in ts.SECTIONS}}
    st.update(changes)
    torch.save(st, path)
    return cfg


def test_file_checks_and_their_messages(tmp_path):
    good = str(tmp_path / "good.pt")
    cfg = _state_file(good)
    st = ts.read(good)
    ts.check_config(st["config"], cfg)
    for field, value in (("learning_rate", 2e-3), ("batch_size", 128), ("p_mode", 1), ("seed", 3)):
        with pytest.raises(ValueError, match=f"{field} is"):
            ts.check_config(st["config"], dict(cfg, **{field: value}))
    bad = str(tmp_path / "bad.pt")
    with open(bad, "wb") as f:
        f.write(b"not a training state")
    with pytest.raises(ValueError, match="not readable"):
        ts.read(bad)
    with pytest.raises(ValueError, match="not readable"):
        ts.read(str(tmp_path / "missing.pt"))
    torch.save({"x": torch.zeros(2)}, bad)
    with pytest.raises(ValueError, match="not a naf-training-state file"):
        ts.read(bad)
    _state_file(bad, version=ts.VERSION + 1)
    with pytest.raises(ValueError, match="format version"):
        ts.read(bad)
    _state_file(bad, abi=3)
    with pytest.raises(ValueError, match="ABI 3"):
        ts.read(bad)
    secs = {s: {"tensors": {}, "meta": {}} for s in ts.SECTIONS if s != "replay"}
    _state_file(bad, sections=secs)
    with pytest.raises(ValueError, match="section 'replay'"):
        ts.read(bad)
    # a section's digest covers its meta and its tensors' dtype, shape and words
    t = {"rows": ("torch.float32", [3, 64], 12345)}
    d = ts.section_digest({"total_added": 3}, t)
    assert d == ts.section_digest({"total_added": 3}, dict(t))
    assert d != ts.section_digest({"total_added": 4}, t)
    assert d != ts.section_digest({"total_added": 3}, {"rows": ("torch.float32", [3, 64], 12346)})
    assert d != ts.section_digest({"total_added": 3}, {"rows": ("torch.float32", [64, 3], 12345)})


def test_loop_position_checks():
    pos = ts.run_position(4, 80, {1: (-3.5, 80), 2: (250.0, 12), 3: (-1.0, 80), 4: (-2.0, 80), 5: (0, 0)})
    assert ts.resume_run(pos, 80, 8) == (4, {1: (-3.5, 80), 2: (250.0, 12), 3: (-1.0, 80), 4: (-2.0, 80)})
    assert ts.resume_run(pos, 80, 4)[0] == 4
    with pytest.raises(ValueError, match="frames is 50"):
        ts.resume_run(pos, 50, 8)
    with pytest.raises(ValueError, match="fewer than the 4"):
        ts.resume_run(pos, 80, 3)
    with pytest.raises(ValueError, match="load a training state"):
        ts.resume_run(None, 80, 8)
    vec = {"tensors": {}, "meta": {"kind": "vectorized", "args": {"n_envs": 64, "max_frames": 16, "robot": "kuka",
                                                                 "drain_every": 8}}}
    with pytest.raises(ValueError, match=r"checkpoint of run\(\)"):
        ts.resume_run(vec, 80, 8)
    for k, v in (("n_envs", 32), ("max_frames", 20), ("robot", "panda"), ("drain_every", 64)):
        args = dict(vec["meta"]["args"], **{k: v})
        with pytest.raises(ValueError, match=f"{k} is"):
            ts.resume_vectorized(vec, None, None, args)
    with pytest.raises(ValueError, match="run_vectorized"):
        ts.resume_vectorized(pos, None, None, vec["meta"]["args"])


class _StubAgent:
    def __init__(self):
        self.calls = []

    def load_training_state(self, path):
        self.calls.append(("load", path))

    def run(self, frames, episodes, verbose, resume=False):
        self.calls.append(("run", frames, episodes, verbose, resume))
        return {}

    def run_vectorized(self, **kw):
        self.calls.append(("run_vectorized", kw["n_envs"], kw["max_frames"], kw["episodes"], kw["resume"]))
        return {"scores": {}}


def test_framework_resume_training_arguments_without_a_gpu(tmp_path, monkeypatch):
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.utils.exceptions import (ConfigurationIncomplete, InvalidNAFAgentParameter,
                                                                MissingWeightsFile)
    monkeypatch.chdir(tmp_path)
    f = ManipulatorFramework()
    with pytest.raises(ConfigurationIncomplete):
        f.resume_training(2, 4)
    f.initialize_synthetic_environment(6)
    with pytest.raises(ConfigurationIncomplete):
        f.resume_training(2, 4)                 # no agent
    f.naf_agent = agent = _StubAgent()
    for episode, episodes in ((0, 4), (2.0, 4), (True, 4), (4, 2), (2, None)):
        with pytest.raises(InvalidNAFAgentParameter):
            f.resume_training(episode, episodes)
    with pytest.raises(MissingWeightsFile, match="training_state.pt"):
        f.resume_training(2, 4)
    os.makedirs("checkpoints/2")
    open("checkpoints/2/training_state.pt", "wb").close()
    f.resume_training(2, 4, frames=80, verbose=False)
    assert agent.calls == [("load", "checkpoints/2/training_state.pt"), ("run", 80, 4, False, True)]
    agent.calls.clear()
    f.resume_training(2, 6, frames=16, verbose=False, n_envs=64)
    assert agent.calls == [("load", "checkpoints/2/training_state.pt"), ("run_vectorized", 64, 16, 6, True)]
    f.env = object()                            # a host environment: its many-env form runs in worker processes
    with pytest.raises(InvalidNAFAgentParameter, match="worker processes"):
        f.resume_training(2, 6, n_envs=4)
