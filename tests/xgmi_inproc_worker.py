"""Worker of tests/test_agent_gpu.py::test_world_8_rehearsal_in_one_process — north_star's only world size, W = 8, executed on a
one-GPU box. The pool allows six processes on a card, so the eight ranks cannot be processes (tests/xgmi_worker.py stops at four):
here they are eight communicators, eight learners and eight streams of ONE process, each rank's receive slab mapped into the others
by plain pointers (naf_xgmi_connect_local) instead of hipIpc. Everything else is the multi-GPU code: xgmi_allreduce_kernel<8> with
its seven flags per rank and the rank-ordered sum of eight, the finish launch's early pushes to seven peers, the exchange inside the
finish launch (`merged`), slots double-buffered by epoch parity, the norm partials, 1 / 8 folded into the clip scale.

    python tests/xgmi_inproc_worker.py [world=8]
A rank's launch waits for its peers' launches, so every stream needs a hardware queue of its own, and the process's queue count is
set by the machine (GPU_MAX_HW_QUEUES), not by this worker. The worker first checks that its eight streams do run side by side
(one all-reduce with a 1-s bound) and prints INPROC_SKIP if not.
Prints INPROC_OK world=<W>; on success.
"""
import os
import sys

ROOT = os.environ.get("NAF_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import torch  # noqa: E402

from robotic_manipulator_rloa_amd import parallel  # noqa: E402


def rank_input(rank, k, n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1000 * k + rank)
    return torch.randn(n, generator=g, device=dev)


def main():
    W = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    streams = [torch.cuda.Stream() for _ in range(W)]

    n = 81152
    # ---- 0. do the streams run side by side? ---------------------------------------------------------------------------------------
    probe = parallel.XgmiAllReduce.local_group(W, n, dev, timeout_s=1.0)
    ones = [torch.full((n,), float(r + 1), device=dev) for r in range(W)]
    res = [torch.empty(n, device=dev) for _ in range(W)]
    torch.cuda.synchronize()
    for _ in range(2):
        for r in range(W):
            with torch.cuda.stream(streams[r]):
                probe[r].all_reduce(ones[r], res[r])
        torch.cuda.synchronize()
    stuck = sum(c.status()[1] for c in probe)
    for c in probe:
        c.close(collective=False)
    if stuck:
        os.write(1, f"INPROC_SKIP the {W} streams of this process share hardware queues ({stuck} timed-out waits in the probe): "
                    f"this process has fewer hardware queues than ranks;".encode())
        return
    # ---- 1. the all-reduce alone: random data, in place / out of place, ranges pushed ahead ----------------------------------
    comms = parallel.XgmiAllReduce.local_group(W, n, dev, timeout_s=20.0)
    outs = [torch.empty(n, device=dev) for _ in range(W)]
    parts = [torch.zeros(comms[0].n_partials, device=dev) for _ in range(W)]
    steps = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(W)]
    rounds = 40
    for k in range(rounds):
        ins = [rank_input(r, k, n, dev) for r in range(W)]
        want = ins[0].clone()
        for r in range(1, W):
            want = want + ins[r]                      # same order and rounding as the kernel's rank-ordered sum
        lo = None
        if k % 4 == 1:
            lo = 4 * (k * 97 % (n // 4))
        torch.cuda.synchronize()
        got = []
        for r in range(W):
            with torch.cuda.stream(streams[r]):
                if lo is not None:
                    comms[r].push_early(ins[r], lo, n)
                if k % 3 == 0:
                    comms[r].all_reduce(ins[r], ins[r], parts[r], steps[r], pushed_lo=lo)
                    got.append(ins[r])
                else:
                    comms[r].all_reduce(ins[r], outs[r], parts[r], steps[r], pushed_lo=lo)
                    got.append(outs[r])
        torch.cuda.synchronize()
        ss = (want.double() ** 2).sum().item()
        for r in range(W):
            assert torch.equal(got[r], want), f"round {k} rank {r}: {(got[r] != want).sum().item()} elements differ"
            assert abs(parts[r].double().sum().item() - ss) < 1e-5 * ss
    for r in range(W):
        epoch, timeouts = comms[r].status()
        assert timeouts == 0 and epoch == rounds and int(steps[r].item()) == rounds, (r, epoch, timeouts)
    for c in comms:
        c.close(collective=False)

    # ---- 2. eight lock-step learners, each with its own minibatches, under both peer-memory forms -----------------------------
    from robotic_manipulator_rloa_amd.engine import UpdateChunk
    from test_learner_gpu import _kuka_learner_and_replay
    B = 64
    for form in ("oneshot", "merged"):
        os.environ["NAF_DP_EXCHANGE"] = form
        Ls, bufs, twins = [], [], []
        probe, _ = _kuka_learner_and_replay(8, B, seed_data=5, learner_kw={"world_size": 1})
        comms = parallel.XgmiAllReduce.local_group(W, probe.lay.P, dev, timeout_s=20.0)
        del probe
        for r in range(W):
            L, buf = _kuka_learner_and_replay(1000, B, seed_data=5 + r, learner_kw={"world_size": W, "_xgmi": comms[r]})
            twin, _ = _kuka_learner_and_replay(8, B, seed_data=5 + r, learner_kw={"world_size": 1})
            assert L.exchange == form and L.xgmi is comms[r] and L.xgmi_merged == (form == "merged")
            Ls.append(L), bufs.append(buf), twins.append(twin)
        # (a) one update: what leaves learn_rows() on every rank is the rank-ordered sum of the eight local gradients (a twin learner
        #     without an exchange, same weights, same rows: the same kernels, bit for bit), the partials its sum of squares
        torch.cuda.synchronize()
        state = [[t.clone() for t in (L.theta2, L.adam_m, L.adam_v, L.bn_stats, L.step_dev)] for L in Ls]
        for r in range(W):
            twins[r].learn_rows(bufs[r].rows[:B])
        torch.cuda.synchronize()
        for r in range(W):
            with torch.cuda.stream(streams[r]):
                Ls[r].learn_rows(bufs[r].rows[:B])
        torch.cuda.synchronize()
        want = twins[0].grad.clone()
        for r in range(1, W):
            want = want + twins[r].grad
        ss = (want.double() ** 2).sum().item()
        for r in range(W):
            L = Ls[r]
            assert torch.equal(L.grad, want), f"{form} rank {r}: {(L.grad != want).sum().item()} elements differ from the rank-ordered sum"
            assert abs(L.partials[:L.n_partials].double().sum().item() - ss) < 1e-5 * ss
            assert int(L.step_dev.item()) == 1 and L.xgmi.status()[1] == 0
            for t, saved in zip((L.theta2, L.adam_m, L.adam_v, L.bn_stats, L.step_dev), state[r]):
                t.copy_(saved)
        del twins
        # (b) 12 updates in chunks of 4 (the optimizer step of update k riding on update k + 1): the replicas stay bit-identical
        chunks = [UpdateChunk(Ls[r], bufs[r], 4, use_graph=False) for r in range(W)]
        torch.cuda.synchronize()
        for _ in range(3):
            for r in range(W):
                with torch.cuda.stream(streams[r]):
                    chunks[r].run()
        torch.cuda.synchronize()
        for r in range(W):
            assert Ls[r].xgmi.status()[1] == 0 and int(Ls[r].step_dev.item()) == 12
            assert torch.equal(Ls[r].theta2, Ls[0].theta2), f"{form}: replica {r} diverged"
            assert torch.isfinite(Ls[r].theta2).all()
        assert not torch.equal(Ls[0].theta2, state[0][0])
        for c in comms:
            c.close(collective=False)
        del Ls, bufs, chunks
    os.write(1, f"INPROC_OK world={W};".encode())


if __name__ == "__main__":
    main()
