"""Training-state numbers on the MI355X: naf_state_digest's bandwidth, and save / load wall time and file size of a full ring.

  python benchmarks/training_state_bench.py [--digest-only]

Digest: the 1 M x 64-float ring of BASELINE configs[1] (256 MiB) and one 1 GiB segment, timed with device events over repeated
launches after a warm-up; share = bytes / time / 8 TB/s (MI355X_MICROARCH.md: 8 TB/s peak). Kernel times for the same
launches: run it under `rocprofv3 --kernel-trace --stats` (--digest-only keeps that run short).
Save / load: NAFAgent.save_training_state / load_training_state of an agent whose ring is full of random rows, at configs[1]
(S = 21, A = 6, B = 256, 1 M rows) and at configs[4]'s ring (S = 23, A = 7, B = 2048, 4 M rows); the file goes to a temporary
directory and is deleted. Prints one JSON line per measurement."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_HBM_GBPS = 8000.0


def digest_bandwidth(reps: int = 20) -> None:
    from robotic_manipulator_rloa_amd.training_state import device_digests
    dev = torch.device("cuda:0")
    for name, words in (("ring_1M_x_64f", (1 << 20) * 64), ("segment_1GiB", (1 << 30) // 4)):
        t = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int32, device=dev)
        for _ in range(3):
            device_digests([t])
        first = device_digests([t])[0]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            device_digests([t])       # (each call reads its result back: the time includes that copy and the memset)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        gbps = 4 * words / ms / 1e6
        print(json.dumps({"measure": "digest", "segment": name, "bytes": 4 * words, "ms_per_call": round(ms, 4),
                          "GB_per_s": round(gbps, 1), "share_of_8TBps": round(gbps / PEAK_HBM_GBPS, 3),
                          "stable": device_digests([t])[0] == first}), flush=True)
        del t


def save_load(tag: str, S: int, A: int, B: int, rows: int) -> None:
    from robotic_manipulator_rloa_amd.naf_components.naf_algorithm import NAFAgent
    d = tempfile.mkdtemp(prefix="naf_ts_")
    old = os.getcwd()
    os.chdir(d)
    try:
        agent = NAFAgent(None, S, A, 256, B, rows, 1e-3, 1e-3, 0.99, 1, 1, 500, torch.device("cuda:0"), 0)
        m = agent.memory
        m.rows.uniform_(-1.0, 1.0)
        m._total_added = rows              # (a full ring: every row is saved)
        torch.cuda.synchronize()
        path = os.path.join(d, "training_state.pt")
        t0 = time.time()
        agent.save_training_state(path)
        t_save = time.time() - t0
        size = os.path.getsize(path)
        other = NAFAgent(None, S, A, 256, B, rows, 1e-3, 1e-3, 0.99, 1, 1, 500, torch.device("cuda:0"), 0)
        torch.cuda.synchronize()
        t0 = time.time()
        other.load_training_state(path)
        torch.cuda.synchronize()
        t_load = time.time() - t0
        same = other.training_state_digest()["replay"] == agent.training_state_digest()["replay"]
        print(json.dumps({"measure": "save_load", "config": tag, "ring_rows": rows, "ring_bytes": m.rows.numel() * 4,
                          "file_bytes": size, "save_s": round(t_save, 2), "load_s": round(t_load, 2), "ring_equal": same}),
              flush=True)
        del agent, other
        torch.cuda.empty_cache()
    finally:
        os.chdir(old)
        shutil.rmtree(d, ignore_errors=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest-only", action="store_true")
    a = ap.parse_args()
    from robotic_manipulator_rloa_amd import _lib
    _lib.require_gpu()
    digest_bandwidth()
    if not a.digest_only:
        save_load("configs[1]", 21, 6, 256, 1 << 20)
        save_load("configs[4] ring", 23, 7, 2048, 4 << 20)


if __name__ == "__main__":
    main()
