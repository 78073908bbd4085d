"""The full training state of a NAFAgent: what the next step of an uninterrupted run reads, moved to and from one file, so that a
resumed run is the same run — same scores, same weights, same actions, to the bit.

Sections (each a dict {"tensors": {name: tensor}, "meta": JSON-able}, each with one 64-bit digest in the file):
  learner  the learner's PUBLIC state: theta2 (main; target), adam_m, adam_v, step_dev, bn_stats
  replay   ring rows [0, min(total_added, capacity)) in physical order, meta {head, size, ...}, the sampler's counter; total_added
  actor    the one-state actor's noise counter; the observation and action a step()'s graph tail has drawn already, if pending
  agent    update_t_step, the data-parallel tick count, the last loss
  rng      Python's `random`, numpy's global generator, torch's CPU generator
  loop     (checkpoints of run / run_vectorized only) where the loop stands

Not saved, and why: the gradient, the norm partials, the prefetched minibatches and every working buffer are speculative — no
schedule leaves an optimizer step pending across step() calls (UpdateChunk's last update and the per-timestep graph's tail
take theirs inside the same run), so the public state is complete between calls. `adam_bc` is a cache of the next step's bias
corrections, tagged with its step number and recomputed by the same function when the tag does not match: not state.

The digest of a tensor is naf_state_digest over its 32-bit words, computed on the device; a section's digest is digest_words_np
over the JSON of its meta and of its tensors' {dtype, shape, digest}. A file is checked in full — format, configuration, shapes,
digests of the uploaded copies — before anything is written into the agent; restore then writes in place, so captured graphs
stay valid, and tells the per-timestep pipeline to start over from public state."""
from __future__ import annotations

import ctypes
import json
import os
import random
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

FORMAT = "naf-training-state"
VERSION = 1
SECTIONS = ("learner", "replay", "actor", "agent", "rng")
CONFIG_FIELDS = ("state_size", "action_size", "layer_size", "batch_size", "buffer_size", "learning_rate", "tau", "gamma",
                 "update_freq", "num_updates", "p_mode", "action_mode", "seed")
_K1, _K2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD6E8FEB86659FD93)
_M64 = (1 << 64) - 1


class _Seg(ctypes.Structure):
    """naf_digest_seg_t (include/naf_hip.h)"""
    _fields_ = [("ptr", ctypes.c_void_p), ("n_words", ctypes.c_uint64)]


# ---- digests -----------------------------------------------------------------------------------------------------------------
def digest_words_np(words: np.ndarray) -> int:
    """naf_state_digest of one segment, on the host: sum over i of mix(i, w_i) mod 2^64 (csrc/state_digest.hip)."""
    w = np.ascontiguousarray(words).view(np.uint32).ravel().astype(np.uint64)
    with np.errstate(over="ignore"):
        x = np.arange(w.size, dtype=np.uint64) * _K1 + w
        x = (x ^ (x >> np.uint64(32))) * _K2
        x ^= x >> np.uint64(32)
        return int(x.sum(dtype=np.uint64))


def digest_bytes(b: bytes) -> int:
    return digest_words_np(np.frombuffer(b + b"\0" * (-len(b) % 4), dtype=np.uint32))


def device_digests(tensors: List[torch.Tensor], blocks_per_seg: int = 0) -> List[int]:
    """One naf_state_digest launch (per 32 segments) over contiguous device tensors whose byte size is a multiple of 4."""
    if not tensors:
        return []
    dev = tensors[0].device
    segs = (_Seg * len(tensors))()
    for i, t in enumerate(tensors):
        if t.device != dev or not t.is_contiguous() or (t.numel() * t.element_size()) % 4:
            raise ValueError("device_digests: contiguous tensors of one device, whole 32-bit words")
        segs[i].ptr, segs[i].n_words = (t.data_ptr() if t.numel() else None), t.numel() * t.element_size() // 4
    out = torch.empty(len(tensors), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().naf_state_digest(segs, len(tensors), out.data_ptr(), int(blocks_per_seg), _lib.stream_ptr()),
               "naf_state_digest")
    return [int(v) & _M64 for v in out.cpu().tolist()]


def _canonical(meta) -> bytes:
    return json.dumps(meta, sort_keys=True, separators=(",", ":")).encode()


def section_digest(meta, tensor_digests: Dict[str, Tuple[str, list, int]]) -> int:
    return digest_bytes(_canonical({"meta": meta, "tensors": {k: list(v) for k, v in sorted(tensor_digests.items())}}))


def digest_sections(sections: dict, device) -> Dict[str, int]:
    """{section: digest}; tensors off the device are uploaded for the kernel."""
    names, ts = [], []
    for s, sec in sections.items():
        for k, t in sec["tensors"].items():
            names.append((s, k, t))
            ts.append(t.to(device).contiguous())
    ds = device_digests(ts)
    per = {s: {} for s in sections}
    for (s, k, t), d in zip(names, ds):
        per[s][k] = (str(t.dtype), list(t.shape), d)
    return {s: section_digest(sections[s]["meta"], per[s]) for s in sections}


# ---- what the agent holds ------------------------------------------------------------------------------------------------------
def agent_config(agent) -> dict:
    return {"state_size": agent.state_size, "action_size": agent.action_size, "layer_size": agent.layer_size,
            "batch_size": agent.batch_size, "buffer_size": agent.buffer_size, "learning_rate": float(agent.learning_rate),
            "tau": float(agent.tau), "gamma": float(agent.gamma), "update_freq": agent.update_freq,
            "num_updates": agent.num_updates, "p_mode": int(agent.learner.p_mode), "action_mode": int(agent.memory.action_mode),
            "seed": agent.seed}


def _require_one_gpu(agent) -> None:
    if agent.world_size > 1:
        raise _lib.NafHipError("training state: data parallel runs (world_size > 1) cannot be saved or resumed")


def _pending_action(agent):
    """(observation, action) the last step()'s graph tail drew for the state the loop asks about next, or None."""
    if agent._restored_ahead is not None:
        return agent._restored_ahead
    if agent._ahead is None:
        return None
    agent._chunk.wait_tail()
    return (np.array(agent._ahead, dtype=np.float32, copy=True), agent._actor1.actions_np[0].copy())


def collect(agent) -> dict:
    """The agent's sections, tensors as they live (device tensors are not copied)."""
    _require_one_gpu(agent)
    L, m = agent.learner, agent.memory
    m.flush()
    if agent._chunk is not None:
        agent._chunk.wait_pinned_free()
    torch.cuda.synchronize()
    n = min(m._total_added, m.buffer_size)
    a = agent._actor1
    ahead = _pending_action(agent)
    actor_t = {"counter": a.counter if a is not None else torch.zeros(1, dtype=torch.int64)}
    if ahead is not None:
        actor_t["ahead_obs"], actor_t["ahead_action"] = torch.from_numpy(ahead[0]), torch.from_numpy(ahead[1])
    loss = None
    if agent._last_loss_from is not None:
        loss = agent.last_loss()
    npst = np.random.get_state()
    pyst = random.getstate()
    return {
        "learner": {"tensors": {"theta2": L.theta2, "adam_m": L.adam_m, "adam_v": L.adam_v, "step_dev": L.step_dev,
                                "bn_stats": L.bn_stats}, "meta": {}},
        "replay": {"tensors": {"rows": m.rows[:n], "meta": m.meta, "sample_ctr": m._sample_ctr},
                   "meta": {"total_added": int(m._total_added), "rows": n}},
        "actor": {"tensors": actor_t, "meta": {"ahead": ahead is not None}},
        "agent": {"tensors": {}, "meta": {"update_t_step": int(agent.update_t_step), "dp_ticks": int(agent._dp_ticks),
                                          "last_loss": loss}},
        "rng": {"tensors": {"torch_cpu": torch.get_rng_state(), "numpy_key": torch.from_numpy(npst[1].astype(np.int64))},
                "meta": {"python": [pyst[0], list(pyst[1]), pyst[2]], "numpy": [npst[0], int(npst[2]), int(npst[3]), float(npst[4])]}},
    }


def save(agent, path: str, loop: Optional[dict] = None) -> None:
    """Write the agent's training state (and, at a loop's checkpoint, where the loop stands) to `path`."""
    sections = collect(agent)
    if loop is not None:
        sections["loop"] = loop
    digests = digest_sections(sections, agent.device)
    out = {"format": FORMAT, "version": VERSION, "abi": int(_lib.load().naf_hip_abi_version()), "config": agent_config(agent),
           "digests": digests,
           "sections": {s: {"tensors": {k: t.detach().cpu() for k, t in sec["tensors"].items()}, "meta": sec["meta"]}
                        for s, sec in sections.items()}}
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    tmp = f"{path}.{os.getpid()}.tmp"
    torch.save(out, tmp)
    os.replace(tmp, path)


# ---- load: check everything, then commit -----------------------------------------------------------------------------------------
def read(path: str) -> dict:
    """torch.load(weights_only=True) + the checks that need no agent: format, version, library ABI, sections present."""
    try:
        st = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        raise ValueError(f"training state {path}: not readable ({type(e).__name__}: {e})") from None
    if not isinstance(st, dict) or st.get("format") != FORMAT:
        raise ValueError(f"training state {path}: not a {FORMAT} file")
    if st.get("version") != VERSION:
        raise ValueError(f"training state {path}: format version {st.get('version')}, this build reads {VERSION}")
    abi = int(_lib.header_abi_version())
    if st.get("abi") != abi:
        raise ValueError(f"training state {path}: written with library ABI {st.get('abi')}, this build is ABI {abi}")
    secs, dig = st.get("sections"), st.get("digests")
    if not isinstance(secs, dict) or not isinstance(dig, dict):
        raise ValueError(f"training state {path}: no sections")
    for s in SECTIONS + (("loop",) if "loop" in secs else ()):
        sec = secs.get(s)
        if not isinstance(sec, dict) or not isinstance(sec.get("tensors"), dict) or "meta" not in sec or s not in dig:
            raise ValueError(f"training state {path}: section '{s}' is missing or malformed")
    return st


def check_config(saved: dict, agent_cfg: dict) -> None:
    if not isinstance(saved, dict):
        raise ValueError("training state: no configuration")
    for k in CONFIG_FIELDS:
        if saved.get(k) != agent_cfg[k]:
            raise ValueError(f"training state: {k} is {saved.get(k)!r} in the file and {agent_cfg[k]!r} in this agent")


def _expect(sec: dict, name: str, like: torch.Tensor, shape=None) -> torch.Tensor:
    t = sec["tensors"].get(name)
    shape = tuple(like.shape) if shape is None else tuple(shape)
    if not isinstance(t, torch.Tensor) or t.dtype != like.dtype or tuple(t.shape) != shape:
        raise ValueError(f"training state: tensor '{name}' is missing or has the wrong dtype / shape "
                         f"(want {like.dtype} {list(shape)})")
    return t


def verify(st: dict, device) -> Dict[str, torch.Tensor]:
    """Upload every tensor and check each section against its digest on the device; returns the uploaded copies."""
    up, per = {}, {s: {} for s in st["sections"]}
    names, ts = [], []
    for s, sec in st["sections"].items():
        for k, t in sec["tensors"].items():
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"training state: section '{s}' holds a non-tensor under '{k}'")
            g = t.to(device).contiguous()
            names.append((s, k, t))
            ts.append(g)
            up[f"{s}.{k}"] = g
    for (s, k, t), d in zip(names, device_digests(ts)):
        per[s][k] = (str(t.dtype), list(t.shape), d)
    for s, sec in st["sections"].items():
        try:
            got = section_digest(sec["meta"], per[s])
        except (TypeError, ValueError):
            got = None
        if got != st["digests"].get(s):
            raise ValueError(f"training state: section '{s}' does not match its digest (the file is corrupt)")
    return up


def load(agent, path: str) -> Optional[dict]:
    """Check the file in full, then restore it into `agent` in place. Returns the loop section (or None)."""
    _require_one_gpu(agent)
    st = read(path)
    check_config(st["config"], agent_config(agent))
    L, m = agent.learner, agent.memory
    secs = st["sections"]
    ln, rp, ac = secs["learner"], secs["replay"], secs["actor"]
    for k in ("theta2", "adam_m", "adam_v", "step_dev", "bn_stats"):
        _expect(ln, k, getattr(L, k))
    n = rp["meta"].get("rows")
    total = rp["meta"].get("total_added")
    if not isinstance(n, int) or not isinstance(total, int) or n != min(total, m.buffer_size) or n < 0:
        raise ValueError("training state: section 'replay' has an inconsistent row count")
    _expect(rp, "rows", m.rows, (n, m.rows.shape[1]))
    _expect(rp, "meta", m.meta)
    _expect(rp, "sample_ctr", m._sample_ctr)
    _expect(ac, "counter", torch.zeros(1, dtype=torch.int64))
    if ac["meta"].get("ahead"):
        _expect(ac, "ahead_obs", torch.zeros(agent.state_size, dtype=torch.float32))
        _expect(ac, "ahead_action", torch.zeros(agent.action_size, dtype=torch.float32))
    up = verify(st, agent.device)
    _commit(agent, st, up)
    return secs.get("loop")


def _commit(agent, st: dict, up: Dict[str, torch.Tensor]) -> None:
    L, m = agent.learner, agent.memory
    secs = st["sections"]
    # nothing of the agent's may still be in flight: a graph's tail reading the pinned row, a prefetch on the side stream
    if agent._chunk is not None:
        agent._chunk.wait_pinned_free()
    m.flush()
    torch.cuda.synchronize()
    with torch.no_grad():
        for k in ("theta2", "adam_m", "adam_v", "step_dev", "bn_stats"):
            getattr(L, k).copy_(up[f"learner.{k}"])
        n = secs["replay"]["meta"]["rows"]
        if n:
            m.rows[:n].copy_(up["replay.rows"])
        m.meta.copy_(up["replay.meta"])
        m._sample_ctr.copy_(up["replay.sample_ctr"])
        agent._actor().counter.copy_(up["actor.counter"])
    L._gen += 1
    m._gen += 1
    m._total_added = secs["replay"]["meta"]["total_added"]
    ch = agent._chunk
    if ch is not None:
        # the per-timestep graph's speculative state was built on what is gone: its prefetch record is void, and the pipelined
        # form starts the next timestep over from public state (its version-counter check would see the copies too)
        if ch.spec_rec is not None:
            ch.spec_rec[0] = 0
        if ch.pipe is not None:
            ch.pipe.spec_rec[:, 0] = 0
            ch.pipe.armed = False
    torch.cuda.synchronize()
    ac = secs["actor"]
    agent._ahead = None
    # step()'s short way skips the learning gate (it is taken only once the gate is open for good): the restored fill level may
    # close it again, so the next step() decides afresh (_row_in_graph) and re-arms the short way when the gate opens
    agent._fast = None
    agent._restored_ahead = ((ac["tensors"]["ahead_obs"].numpy().copy(), ac["tensors"]["ahead_action"].numpy().copy())
                             if ac["meta"]["ahead"] else None)
    am = secs["agent"]["meta"]
    agent.update_t_step, agent._dp_ticks = int(am["update_t_step"]), int(am["dp_ticks"])
    agent._restored_loss = am["last_loss"]
    agent._last_loss_from = "restored" if am["last_loss"] is not None else None
    rg = secs["rng"]
    py = rg["meta"]["python"]
    random.setstate((py[0], tuple(py[1]), py[2]))
    nm = rg["meta"]["numpy"]
    np.random.set_state((nm[0], rg["tensors"]["numpy_key"].numpy().astype(np.uint32), nm[1], nm[2], nm[3]))
    torch.set_rng_state(rg["tensors"]["torch_cpu"])


# ---- loop positions ------------------------------------------------------------------------------------------------------------
def run_position(episode: int, frames: int, scores: dict) -> dict:
    return {"tensors": {}, "meta": {"kind": "run", "episode": int(episode), "frames": int(frames),
                                    "scores": [[int(e), s if isinstance(s, int) else float(s), int(f)]
                                               for e, (s, f) in scores.items() if e <= episode]}}


def resume_run(loop: Optional[dict], frames: int, episodes: int) -> Tuple[int, dict]:
    """(episodes done, {episode: (score, frames)} so far) from the loop section a checkpoint of run() left."""
    if loop is None or loop["meta"].get("kind") != "run":
        raise ValueError("run(resume=True): load a training state written at a checkpoint of run() first")
    lm = loop["meta"]
    if lm["frames"] != frames:
        raise ValueError(f"run(resume=True): frames is {frames}, the saved run used {lm['frames']}")
    if episodes < lm["episode"]:
        raise ValueError(f"run(resume=True): episodes = {episodes} is fewer than the {lm['episode']} the saved run has done")
    return lm["episode"], {e: (s, f) for e, s, f in lm["scores"]}


def vectorized_position(loop_env, ledger, dropped: List[Tuple[float, int]], steps: int, updates: int, args: dict) -> dict:
    """At a drain: the device envs, the record copy not parsed yet, the ledger and the counters of run_vectorized."""
    t = {"env_state": loop_env.env_state, "obs": loop_env.actor.obs, "counter": loop_env.actor.counter,
         "step_ctr": loop_env.step_ctr, "records": loop_env.records}
    inflight = None
    if loop_env._inflight is not None:
        pin, ev, first, n = loop_env._inflight
        ev.synchronize()
        t["inflight"] = pin
        inflight = [int(first), int(n)]
    return {"tensors": t, "meta": {
        "kind": "vectorized", "args": args, "steps": int(steps), "updates": int(updates), "loop_steps": int(loop_env._steps),
        "copied": int(loop_env._copied), "env_steps": int(loop_env.env_steps), "inflight": inflight,
        "ledger": {"count": ledger.count, "extra": ledger.extra, "checkpoints": list(ledger.checkpoints),
                   "scores": [[int(e), float(s), int(f)] for e, (s, f) in ledger.scores.items() if e <= ledger.count],
                   "dropped": [[float(s), int(f)] for s, f in dropped]}}}


def resume_vectorized(loop: Optional[dict], loop_env, ledger, args: dict) -> Tuple[int, int, List[Tuple[float, int]]]:
    """Put run_vectorized's loop back where the checkpoint left it; returns (steps, updates, episodes the saved run's budget
    had left unrecorded — the caller books them into a larger budget)."""
    if loop is None or loop["meta"].get("kind") != "vectorized":
        raise ValueError("run_vectorized(resume=True): load a training state written at a checkpoint of run_vectorized() first")
    lm = loop["meta"]
    for k in lm["args"]:
        if k not in args:                  # (a chain model's run loaded into a stand-in's: 'chain', 'scene')
            raise ValueError(f"run_vectorized(resume=True): the saved run used {k} = {lm['args'][k]!r}, this one has none")
    for k, v in args.items():
        if lm["args"].get(k) != v:
            raise ValueError(f"run_vectorized(resume=True): {k} is {v!r}, the saved run used {lm['args'].get(k)!r}")
    lg = lm["ledger"]
    if ledger.limit is not None and ledger.limit < lg["count"]:
        raise ValueError(f"run_vectorized(resume=True): episodes = {ledger.limit} is fewer than the {lg['count']} "
                         "the saved run has recorded")
    dev = loop_env.env_state.device
    with torch.no_grad():
        for k, live in (("env_state", loop_env.env_state), ("obs", loop_env.actor.obs), ("counter", loop_env.actor.counter),
                        ("step_ctr", loop_env.step_ctr), ("records", loop_env.records)):
            t = loop["tensors"].get(k)
            if not isinstance(t, torch.Tensor) or t.shape != live.shape or t.dtype != live.dtype:
                raise ValueError(f"training state: loop tensor '{k}' does not fit this loop")
            live.copy_(t.to(dev))
    loop_env._steps, loop_env._copied, loop_env.env_steps = lm["loop_steps"], lm["copied"], lm["env_steps"]
    loop_env._finished = []
    loop_env._inflight = None
    if lm["inflight"] is not None:
        pin = loop_env._pins[1]
        pin.copy_(loop["tensors"]["inflight"])
        ev = torch.cuda.Event()
        ev.record()
        loop_env._pin_i = 0
        loop_env._inflight = (pin, ev, lm["inflight"][0], lm["inflight"][1])
    for e, s, f in lg["scores"]:
        ledger.scores[e] = (s, f)
    ledger.count, ledger.extra, ledger.checkpoints = lg["count"], lg["extra"], list(lg["checkpoints"])
    dropped = [(s, f) for s, f in lg["dropped"]]
    ledger.extra -= len(dropped)            # (booked again by the caller: recorded now if the budget has room)
    torch.cuda.synchronize()
    return lm["steps"], lm["updates"], dropped
