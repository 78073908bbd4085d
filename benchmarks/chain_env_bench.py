"""Vectorized training rate of the kinematic chain environment (csrc/chain_env.hip) beside the stand-in's at the same joint
count, a launch loop of the two step kernels for `rocprofv3 --kernel-trace --stats`, and the step and rollout-step launches timed.

  python benchmarks/chain_env_bench.py rate --urdf tests/golden/urdf/iiwa_like7.urdf --steps 4000 --warmup 100
      env-steps/s of NAFAgent.run_vectorized, E = 64, B = 256: the chain environment, then the stand-in at the same A
      (`--standin-only`: only the latter — what a tree without the chain environment can run; `--autocollision`: the chain
      environment compiled with consider_autocollision=True, `--arm standin8`: a fixture arm with its full joint count)
  rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/chain_env_bench.py kernels
      1000 launches each of chain_env_step_kernel for standin8 (A = 8, E = 64) and long32, and of synth_env_step_kernel
      (`--autocollision`: the two arms compiled with their self-collision pairs, 18 and 465: the SC = true instantiation)
  python benchmarks/chain_env_bench.py step --envs 4096 --launches 4000 [--autocollision] [--workcell [--boxes]]
      microseconds per naf_chain_env_step launch of --urdf (device events around `--launches` launches with the step counter
      running, max_frames = 400, N(0, 1) actions; `--repeats` windows after one warm-up window). Two launches per step are
      enqueued by the host, so at small E the figure is bounded below by launch submission: the kernel's own time comes from
      `rocprofv3 --kernel-trace --stats -d OUT -- python benchmarks/chain_env_bench.py step ...`, a run of its own, whose
      maximum per kernel is the launch in which the envs reset (every 400th).

  python benchmarks/chain_env_bench.py rollout --envs 4096 --launches 4000 [--autocollision] [--workcell [--boxes]]
      microseconds per naf_chain_env_rollout_step launch of --urdf, measured as `step` measures (the same arm, start pose and seeded
      N(0, 1) actions; ONE launch per step: there is no counter), after naf_chain_env_reset_given at the start pose with target and
      obstacle 3 m away and a frame budget beyond the run, so that every env stays live: a held lane returns at once and would
      flatter the figure. `--trajectory`: the joint values of a window of frames are recorded too (the budget is then the window).

`--workcell` (step, rollout): the chain model gets a floor under the base and two spheres beside the arm, so the launches are the
workcell instantiations. In a rollout an env that touches one of them is held from then on: `envs_held_before_the_window_ended`
says how many did. `--workcell --boxes` adds three boxes to them — a table top beside the base, a shelf, a rounded post — so the
launches are the box instantiations, which test the floor and the spheres too.

  python benchmarks/chain_env_bench.py gather [--hindsight 0.8] [--horizon 400] [--launches 200]
      microseconds per launch of the replay gather at n = 64 x 256 rows of the S = 23 / A = 7 arm (--urdf), between device events
      around every single launch (median and minimum of `--launches` launches after 20 unmeasured ones), on a ring that
      DeviceEnvLoop(tag_rows=True) filled with `--steps` vector steps of E = `--envs` envs under the untrained policy: the plain
      gather (naf_replay_gather_rows) and the hindsight gather at the given ratio and horizon, interleaved, on the same indices;
      and the hindsight kernel's registers and scratch as the compiler reported them.

  python benchmarks/chain_env_bench.py ik [--envs 4096] [--launches 20]
      goal poses for N = --envs targets (default 4096 here), R = 8 restarts, K = 32 updates, on --urdf with self-collision inside
      the --workcell --boxes cell (always on for this subcommand), targets uniform in a box around the nominal one:
      microseconds per naf_chain_ik_solve launch and milliseconds per whole GoalPoseSolver.solve call (host seeds, uploads,
      solve -> reset_given -> probes -> select, downloads), each between device events, median and minimum of `--launches` after
      two unmeasured ones; the reachable and free shares; and the float64 host twin's seconds on the first 64 of the queries,
      with its time for all N EXTRAPOLATED from those 64 (it is linear in N) — that figure is not a measurement.
      `--avoid-contact`: also the shares and the whole call's time with solve(avoid_contact=True), and naf_chain_ik_clear (16
      updates on the solved candidates) timed alternating, launch by launch in this process, with naf_chain_ik_solve at the same
      16 updates and with reset_given + probe + probe_cell over the same candidates.

  python benchmarks/chain_env_bench.py path [--envs 2048] [--launches 20] [--boxes] [--certify | --roadmap M]
      collision-checked joint paths on --urdf with self-collision inside the --workcell cell (always on for this subcommand): N =
      --envs queries (default 2048 here) x C = 16 candidate vias x S = 256 samples. Microseconds per naf_chain_path_check launch
      between device events (median and minimum of `--launches` after two unmeasured ones), and in the same process the
      composition it replaces — naf_chain_env_reset_given + naf_chain_env_probe + naf_chain_env_probe_cell at E = N C S over the
      materialised poses (the fused launch's own poses_out), in chunks of 2^20 envs — with the bytes each form allocates and the
      largest difference between their minima. Then the README's question on 2000 targets around the nominal one: the goal poses
      (GoalPoseSolver), the paths to them (JointPathChecker, 16 candidates, resolution 0.02) and the shares of 'straight' / 'via' /
      'blocked' among the queries with a free goal pose.
      --certify: instead, microseconds per naf_chain_path_certify launch and per naf_chain_path_check launch on the same inputs,
      alternating in the same process, with their ratio and the share of certified candidates; then the README's question with
      JointPathChecker(certify=True): the shares of 'straight' / 'via' / 'sampled' / 'blocked', the distribution of `refinements`
      and the seconds all rounds took together.

      --roadmap M: instead, microseconds per naf_chain_edge_check launch beside the naf_chain_path_check launch, alternating in
      the same process: the roadmaps (start, goal and M milestones, all their E edges) of as many of the N queries as give the
      path launch's number of workgroups or fewer, at the same S = 256, with both launches' time per sample. Then the README's
      question with and without JointPathChecker.check(roadmap=M): the outcome shares among the queries with a free goal pose,
      how many 'blocked' ones the roadmap turned into 'roadmap', the node counts of those, and the seconds each call took.
      --roadmap M --shortcut W: the question a third time with check(roadmap=M, shortcut=W), and under "shortcut" the 'roadmap'
      polylines before and after the round: length over the straight line, node counts, planned ticks at speed 1, and how their
      demonstrations along all legs (demonstration_plan_legs, frames = 400, through DemonstrationWriter) end.

  python benchmarks/chain_env_bench.py edgecert [--launches 20] [--boxes] [--roadmap 14] [--shortcut 16]
      certificates for roadmap and shortcut polylines, same arm and cell. Microseconds per naf_chain_edge_certify launch beside the
      naf_chain_edge_check launch over the same nodes and edges, alternating in the same process (median and minimum of
      `--launches`, at most 50, after two unmeasured ones), at two shapes: the README's roadmaps (273 roadmaps x all 120 edges of
      M = 14 milestones x 256 samples) and the polyline shape (the same 273 x 16 nodes, the 15 legs (l, l + 1) only), with their
      ratios and the new kernels' registers. Then the README's 'roadmap' polylines (JointPathChecker.check(roadmap=M) on 2000
      targets, and again with shortcut=W) through PolylineCertifier.certify at clearance_margin 0 and at 2e-4 A reach: how many end
      'certified', 'sampled' and 'blocked', the distribution of `refinements`, the launches and the seconds each call took.

  python benchmarks/chain_env_bench.py demo [--envs 2048] [--launches 20] [--boxes]
      planned joint paths as replay rows, same arm and cell: N = --envs demonstrations (default 2048 here) of T = 400 ticks.
      Microseconds per naf_chain_demo_rows launch between device events (median and minimum of `--launches`, at most 30, after two
      unmeasured ones), and in the same process the composed form it replaces — 400 x naf_chain_env_step at E = N behind one
      naf_chain_env_reset_given, the actions already on the device — with their ratio, the mean number of valid rows, the shares of
      the end codes and the new kernels' registers.
      --legs K: instead, microseconds per naf_chain_demo_rows_legs launch beside the naf_chain_demo_rows launch, alternating in the
      same process, on the same two-leg plans: the legs launch takes them split into K legs of the same actions, and the valid rows
      and records of the two are compared to the bit.

  python benchmarks/chain_env_bench.py line [--envs 2048] [--launches 20] [--workcell [--boxes]]
      straight-line end-effector moves, same arm (with self-collision; the cell only where asked for): N = --envs lines (default 2048 here) of W = 32 waypoints x U = 4 updates
      from approach-from-above goal poses, 8 cm straight up. Microseconds per naf_chain_line_track launch between device events
      in the modes full (orientation held) and position, each beside its yardstick — naf_chain_ik_solve_pose / naf_chain_ik_solve at
      N x 1 candidates and W U = 128 iterations: the same number of the same updates in the same number of waves — the two
      alternating launch by launch in the same process (median and minimum of `--launches`, at most 50, after two unmeasured
      ones), with their ratios and the new kernels' registers. Then the whole ManipulatorFramework.plan_linear_moves call (upload,
      tracking launch, download, verdict, the legs' edge launch, gather) in host milliseconds, and the outcomes it reports.

  python benchmarks/chain_env_bench.py traj [--launches 20] [--certify] [--boxes] [--envs 2048]
      time-parameterised trajectories, same arm (with self-collision, the floor and the two spheres): N = --envs targets (default
      2048 here) around the nominal one, their paths planned with --roadmap 14 --shortcut 16, driven at vmax 1 rad/s, amax 4 rad/s^2
      and the environment's tick. Microseconds per naf_chain_traj_check launch between device events beside naf_chain_edge_check
      over the SAME number of walked poses — as many items, E = ticks / 256 edges of 256 samples each — alternating launch by
      launch in the same process (median and minimum of `--launches`, at most 50, after two unmeasured ones), with the ratio;
      --certify: the same for naf_chain_traj_certify beside naf_chain_edge_certify. Then what the trajectories of the free
      polylines come to, what those of the certified polylines come to under certify at the same margin, the durations against a
      stop at every corner, and the new kernels' registers.

`--hindsight R` (rate): the chain runs relabel a share R of every minibatch (NAFAgent.run_vectorized(hindsight=R)). Such a run
wants an empty ring, so with the flag — also `--hindsight 0`, the figure to compare with — the warm-up steps run on an agent of
their own and the timed run starts on a fresh one (its graph captures are inside the timed window, in both).

`--target-range X Y Z` / `--obstacle-range X Y Z` (rate, step): half-widths of the boxes every episode draws its target / obstacle
from (include/naf_hip.h, "Scene ranges"); step then also prints how the episode starts of the run chose their scenes.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
URDF = os.path.join(ROOT, "tests", "golden", "urdf")


def rate(a):
    import torch
    from robotic_manipulator_rloa_amd.environment.synthetic import SyntheticEnvironment
    from robotic_manipulator_rloa_amd.naf_components.naf_algorithm import NAFAgent
    dev = torch.device("cuda:0")
    os.chdir(tempfile.mkdtemp())
    out = {}

    def run(tag, env, A, **kw):
        agent = NAFAgent(env, 2 * A + 9, A, 256, a.batch, 1_000_000, 1e-3, 1e-3, 0.99, 1, 1, 10 ** 9, dev, 0)
        if a.hindsight is not None and "chain" in kw:
            kw = dict(kw, hindsight=a.hindsight, hindsight_horizon=a.horizon)
            agent.run_vectorized(a.warmup, n_envs=a.envs, max_frames=400, **kw)
            agent = NAFAgent(env, 2 * A + 9, A, 256, a.batch, 1_000_000, 1e-3, 1e-3, 0.99, 1, 1, 10 ** 9, dev, 0)
        else:
            agent.run_vectorized(a.warmup, n_envs=a.envs, max_frames=400, **kw)
        r = agent.run_vectorized(a.steps, n_envs=a.envs, max_frames=400, **kw)
        out[tag] = {"env_steps_per_s": round(r["env_steps_per_s"], 1), "updates": r["updates"], "seconds": round(r["seconds"], 4)}
        out[tag].update({k: round(v, 4) for k, v in r.items() if k.startswith("hindsight")})

    if not a.standin_only:
        from robotic_manipulator_rloa_amd.environment.kinematic import build_kinematic
        n = a.joints
        if a.arm:        # a fixture arm: every joint driven, none held (standin8, long12: serial chains without fixed joints)
            env = build_kinematic(os.path.join(URDF, a.arm + ".urdf"), n - 1, [], list(range(n)), [0.4, 0.85, 0.71], [0.45, 0.55, 0.55],
                                  ([0.9, 0.45] + [0.0] * n)[:n], [0.1] * n, 0.03, consider_autocollision=a.autocollision)
        else:
            env = build_kinematic(os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf), n - 1, [n],
                                  list(range(n)), [0.45, 0.3, 0.6], [0.35, 0.2, 0.45], [0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0][:n],
                                  [0.1] * n, 0.03, consider_autocollision=a.autocollision)
        out["self_pairs"] = len(env.model.self_pairs)
        for rep in range(a.repeats):
            run(f"chain_{rep}", env, n, chain=env.model,
                scene={"target": [0.45, 0.3, 0.6], "obstacle": [0.35, 0.2, 0.45], **_ranges(a)})
            run(f"standin_{rep}", SyntheticEnvironment(n), n, robot="panda")
    else:
        for rep in range(a.repeats):
            run(f"standin_{rep}", SyntheticEnvironment(a.joints), a.joints, robot="panda")
    print(json.dumps({"envs": a.envs, "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "joints": a.joints,
                      "hindsight": a.hindsight, **out}))


def _workcell(a) -> dict:
    """--workcell: a floor under the base and two spheres beside the arm (compile_chain's arguments), clear of the start pose"""
    if a.boxes and not a.workcell:
        raise SystemExit("--boxes adds to --workcell: give both")
    if not a.workcell:
        return {}
    cell = {"floor_height": 0.0, "workcell_spheres": [(0.51, 0.38, 0.64, 0.128), (-0.4, -0.4, 0.5, 0.1)]}
    if a.boxes:      # a table top, a shelf, a post (a capsule: zero half extents across, a rounding radius)
        cell["workcell_boxes"] = [(0.58, -0.45, 0.19, 0.32, 0.2, 0.026, 0.0, 0.0, 0.3), (-0.13, 0.64, 0.77, 0.26, 0.064, 0.19, 0.4, -0.3, 0.8),
                                  (0.0, -0.58, 0.9, 0.0, 0.0, 0.38, 1.2, 0.2, 0.0, 0.05)]
    return cell


def _ranges(a) -> dict:
    if a.target_range is None and a.obstacle_range is None:
        return {}
    return {"target_range": a.target_range or [0.0] * 3, "obstacle_range": a.obstacle_range or [0.0] * 3}


def step(a):
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.environment.urdf_chain import compile_chain, load_urdf
    lib = _lib.load()
    dev = torch.device("cuda:0")
    E, n, stream = a.envs, a.joints, torch.cuda.current_stream().cuda_stream
    urdf = os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf)
    # the start pose and reset ranges of the README's example on the first seven joints, 0 +- 0.1 on any further one
    init = ([0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0] + [0.0] * n)[:n]
    var = ([0.1, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2] + [0.1] * n)[:n]
    model = compile_chain(load_urdf(urdf), n - 1, list(range(n)), [n], init, var, 0.03, consider_autocollision=a.autocollision,
                          **_workcell(a))
    blob = np.ascontiguousarray(model.pack())
    h = ctypes.c_void_p()
    _lib.check(lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(h)), "create")
    S = 2 * n + 9
    st = torch.zeros(E, lib.naf_chain_env_state_floats(h), device=dev)
    torch.manual_seed(5)                                  # the same actions in every run: runs of two builds do the same work
    obs, act = torch.zeros(E, S, device=dev), torch.randn(E, n, device=dev)
    rows = torch.zeros(E, lib.naf_replay_row_floats(S, n), device=dev)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    centre = [0.45, 0.3, 0.6, 0.35, 0.2, 0.45]
    scene = (ctypes.c_float * 8)(*centre, 0.0, 0.06)
    ranges = _ranges(a)
    if ranges:
        r7 = (ctypes.c_float * 7)(*ranges["target_range"], *ranges["obstacle_range"], 0.02)
        _lib.check(lib.naf_chain_env_set_scene_ranges(h, r7), "set_scene_ranges")
    _lib.check(lib.naf_chain_env_reset(h, st.data_ptr(), obs.data_ptr(), E, scene, 5, 0, stream), "reset")
    times, starts = [], 0
    for w in range(a.repeats + 1):                        # window 0 warms up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        before = st[:, n + 8].sum().item()
        t0.record()
        for _ in range(a.launches):
            _lib.check(lib.naf_chain_env_step(h, st.data_ptr(), act.data_ptr(), rows.data_ptr(), obs.data_ptr(), E, 5, ctr.data_ptr(),
                                              400, None, 0, stream), "step")
            _lib.check(lib.naf_counter_add(ctr.data_ptr(), 1, stream), "counter_add")
        t1.record()
        torch.cuda.synchronize()
        if w:
            times.append(round(1e3 * t0.elapsed_time(t1) / a.launches, 3))
        starts += int(st[:, n + 8].sum().item() - before)
    out = {"arm": os.path.basename(urdf), "envs": E, "autocollision": a.autocollision, "self_pairs": len(model.self_pairs),
           "workcell_pairs": len(model.cell_pairs), "boxes": len(model.cell_boxes), "launches": a.launches, "ranges": ranges or None, "us_per_step_and_counter_launch": times, "episode_starts": starts}
    if ranges:      # the scenes the envs hold now: the centres, exactly, are fallbacks
        s = st[:, n:n + 6].cpu().numpy()
        out["fallback_share_now"] = round(float(np.mean(np.all(s == np.float32(centre), axis=1))), 4)
    lib.naf_chain_env_destroy(h)
    print(json.dumps(out))


def rollout(a):
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.environment.urdf_chain import compile_chain, load_urdf
    lib = _lib.load()
    dev = torch.device("cuda:0")
    E, n, stream = a.envs, a.joints, torch.cuda.current_stream().cuda_stream
    urdf = os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf)
    init = ([0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0] + [0.0] * n)[:n]             # step's arm and start pose
    var = ([0.1, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2] + [0.1] * n)[:n]
    model = compile_chain(load_urdf(urdf), n - 1, list(range(n)), [n], init, var, 0.03, consider_autocollision=a.autocollision,
                          **_workcell(a))
    blob = np.ascontiguousarray(model.pack())
    h = ctypes.c_void_p()
    _lib.check(lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(h)), "create")
    S = 2 * n + 9
    st = torch.zeros(E, lib.naf_chain_env_state_floats(h), device=dev)
    torch.manual_seed(5)
    obs, act = torch.zeros(E, S, device=dev), torch.randn(E, n, device=dev)
    outcome = torch.zeros(E, 8, device=dev)
    q0 = torch.tensor(init, device=dev).repeat(E, 1).contiguous()
    scene = torch.tensor([0.0, 0.0, 3.0, 0.0, 0.0, -3.0], device=dev).repeat(E, 1).contiguous()
    budget = a.launches if a.trajectory else a.launches * (a.repeats + 1) + 1
    traj = torch.zeros(budget + 1, E, n, device=dev) if a.trajectory else None
    times, held = [], []
    for w in range(a.repeats + 1):                        # window 0 warms up
        if w == 0 or a.trajectory:
            _lib.check(lib.naf_chain_env_reset_given(h, st.data_ptr(), obs.data_ptr(), E, q0.data_ptr(), scene.data_ptr(), 0.06,
                                                     stream), "reset_given")
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            _lib.check(lib.naf_chain_env_rollout_step(h, st.data_ptr(), act.data_ptr(), obs.data_ptr(), outcome.data_ptr(),
                                                      traj.data_ptr() if traj is not None else None, E, budget, stream), "rollout_step")
        t1.record()
        torch.cuda.synchronize()
        if w:
            times.append(round(1e3 * t0.elapsed_time(t1) / a.launches, 3))
            # envs that ended before the window's last launch idled in it
            held.append(int(((outcome[:, 0] != 0) | (outcome[:, 1] < (a.launches if a.trajectory else a.launches * (w + 1)))).sum().item()))
    lib.naf_chain_env_destroy(h)
    print(json.dumps({"arm": os.path.basename(urdf), "envs": E, "autocollision": a.autocollision, "self_pairs": len(model.self_pairs),
                      "workcell_pairs": len(model.cell_pairs), "boxes": len(model.cell_boxes), "launches": a.launches, "trajectory": bool(a.trajectory), "us_per_rollout_step_launch": times,
                      "envs_held_before_the_window_ended": held}))


def gather(a):
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.engine import DeviceEnvLoop
    from robotic_manipulator_rloa_amd.environment.kinematic import build_kinematic
    from robotic_manipulator_rloa_amd.naf_components.naf_algorithm import NAFAgent
    dev = torch.device("cuda:0")
    os.chdir(tempfile.mkdtemp())
    n = a.joints
    env = build_kinematic(os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf), n - 1, [n], list(range(n)),
                          [0.45, 0.3, 0.6], [0.35, 0.2, 0.45], [0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0][:n], [0.1] * n, 0.03)
    U, B, E = 64, 256, a.envs
    agent = NAFAgent(env, 2 * n + 9, n, 256, B, 1_000_000, 1e-3, 1e-3, 0.99, 1, 1, 10 ** 9, dev, 0)
    mem = agent.memory
    loop = DeviceEnvLoop(agent.learner, mem, E, seed=1, max_frames=400, chain=env.model, target=[0.45, 0.3, 0.6],
                         obstacle=[0.35, 0.2, 0.45], target_range=a.target_range or [0.15, 0.15, 0.1], tag_rows=True)
    for _ in range(a.steps):
        loop.step()
    idx = torch.zeros(U, B, dtype=torch.int32, device=dev)
    mem.sample_indices(idx, U)
    rows = torch.zeros(U * B, mem.batch_row_floats, device=dev)
    k_out = torch.zeros(U * B, dtype=torch.int32, device=dev)
    ratio = 0.8 if a.hindsight is None else a.hindsight
    horizon = 400 if a.horizon is None else a.horizon
    forms = {"plain": lambda: mem.gather_rows(idx, rows, U * B),
             "hindsight": lambda: mem.gather_rows_hindsight(idx, rows, U * B, E, horizon, ratio, B, -U, k_out)}
    times = {k: [] for k in forms}
    for i in range(a.launches + 20):
        for k, f in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            if i >= 20:
                times[k].append(1e3 * t0.elapsed_time(t1))
    k = k_out.cpu().numpy()
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name.split("kernelILi")[1].split("E")[0]: {q: v[q] for q in ("vgprs", "sgprs", "scratch_bytes_per_lane")}
            for name, v in usage.items() if "replay_gather_rows_hindsight_kernel" in name}
    print(json.dumps({"rows": U * B, "ring_rows": len(mem), "envs": E, "ratio": ratio, "horizon": horizon, "launches": a.launches,
                      "us_per_launch": {k: {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2)} for k, v in times.items()},
                      "relabelled_share": round(float(np.mean(k >= 0)), 4), "no_valid_candidate_share": round(float(np.mean(k == -2)), 4),
                      "hindsight_kernel_registers_by_width": regs}))


def ik(a):
    import time
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    from robotic_manipulator_rloa_amd.environment.kinematic import KinematicEnvironment, goal_poses_host
    from robotic_manipulator_rloa_amd.environment.urdf_chain import compile_chain, load_urdf
    N, R, K, n = (4096 if a.envs == 64 else a.envs), 8, 32, a.joints
    a.workcell = a.boxes = True
    urdf = os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf)
    init = ([0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0] + [0.0] * n)[:n]
    model = compile_chain(load_urdf(urdf), n - 1, list(range(n)), [n], init, [0.1] * n, 0.03, consider_autocollision=True, **_workcell(a))
    rng = np.random.default_rng(5)
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.25, 0.25, (N, 3))
    obstacles, q0 = np.tile([0.35, 0.2, 0.45], (N, 1)), np.tile(init, (N, 1))
    solver = GoalPoseSolver(model, 0.06)
    whole, kernel = [], []
    for i in range(a.launches + 2):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = solver.solve(q0, targets, obstacles, restarts=R, iterations=K)
        t1.record()
        t1.synchronize()
        if i >= 2:
            whole.append(t0.elapsed_time(t1))
    prm = solver.params(K)                                   # the last chunk's queries are still in the buffers
    per = min(N, solver.chunk // R)
    for i in range(a.launches + 2):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        solver.launch(per, R, prm, 1e-3, 0.0, solve_only=True)
        t1.record()
        t1.synchronize()
        if i >= 2:
            kernel.append(1e3 * t0.elapsed_time(t1))
    oriented = _ik_oriented(a, solver, q0, targets, obstacles, R, K, per, prm) if a.orientation else None
    pushed = _ik_avoid_contact(a, solver, q0, targets, obstacles, R, K, per) if a.avoid_contact else None
    twin = KinematicEnvironment(model, (0.45, 0.3, 0.6), (0.35, 0.2, 0.45), 0.06)
    t = time.perf_counter()
    host = goal_poses_host(twin, q0[:64], targets[:64], obstacles[:64], restarts=R, iterations=K)
    twin_s = time.perf_counter() - t
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "occupancy")} for name, v in usage.items()
            if "chain_ik_" in name}
    print(json.dumps({"arm": os.path.basename(urdf), "queries": N, "restarts": R, "iterations": K, "self_pairs": len(model.self_pairs),
                      "workcell_pairs": len(model.cell_pairs), "candidates_per_solve_launch": per * R,
                      "us_per_ik_solve_launch": {"median": round(float(np.median(kernel)), 1), "min": round(float(np.min(kernel)), 1)},
                      "ms_per_solve_goal_poses_call": {"median": round(float(np.median(whole)), 2), "min": round(float(np.min(whole)), 2)},
                      "reachable_share": round(float(out.reachable.mean()), 4), "free_share": round(float(out.free.mean()), 4),
                      "twin_seconds_for_64_queries": round(twin_s, 3),
                      "twin_seconds_for_all_queries_EXTRAPOLATED_from_64": round(twin_s * N / 64, 1),
                      "twin_and_device_agree_on_reachable_of_64": int(np.sum(host.reachable == out.reachable[:64])),
                      "kernel_registers": regs, **({"orientation": oriented} if oriented else {}),
                      **({"avoid_contact": pushed} if pushed else {})}))


def _ik_avoid_contact(a, solver, q0, targets, obstacles, R, K, per) -> dict:
    """ik --avoid-contact: the same queries with the null-space push — the shares and the whole call's time, then three launches
    timed alternating in this process on the last chunk's candidates: naf_chain_ik_clear, naf_chain_ik_solve at the same trip count,
    and reset_given + probe + probe_cell."""
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd._lib import check, ptr, stream_ptr
    whole = []
    for i in range(a.launches + 2):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = solver.solve(q0, targets, obstacles, restarts=R, iterations=K, avoid_contact=True)
        t1.record()
        t1.synchronize()
        if i >= 2:
            whole.append(t0.elapsed_time(t1))
    clear = solver.clear_params(1e-3)
    short, E = solver.params(clear[0].iterations), per * R
    solver.launch(per, R, solver.params(K), 1e-3, 0.0, solve_only=True)      # the candidates the clear launch works on
    solved = solver.q.clone()

    def probes():
        st = stream_ptr()
        check(solver.lib.naf_chain_env_reset_given(solver._chain_env, ptr(solver.env_state), ptr(solver.obs), E, ptr(solver.q),
                                                   ptr(solver.scene), solver.obstacle_radius, st), "reset_given")
        check(solver.lib.naf_chain_env_probe(solver._chain_env, ptr(solver.env_state), ptr(solver.probe), E, st), "probe")
        check(solver.lib.naf_chain_env_probe_cell(solver._chain_env, ptr(solver.env_state), ptr(solver.cell), E, st), "probe_cell")

    def clear_launch():
        solver.q.copy_(solved)                                               # (in place: every launch refines the solved poses)
        return lambda: solver.launch_clear(per, R, clear)
    kinds = {"clear": clear_launch, "solve_same_updates": lambda: (lambda: solver.launch(per, R, short, 1e-3, 0.0, solve_only=True)),
             "reset_given_and_probes": lambda: probes}
    times = {k: [] for k in kinds}
    for i in range(3 * (a.launches + 2)):
        which = list(kinds)[i % 3]
        run = kinds[which]()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run()
        t1.record()
        t1.synchronize()
        if i >= 6:
            times[which].append(1e3 * t0.elapsed_time(t1))
    stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1)}      # noqa: E731
    return {"updates": int(clear[0].iterations), "candidates": E, "us_per_ik_clear_launch": stat(times["clear"]),
            "us_per_ik_solve_launch_same_updates": stat(times["solve_same_updates"]),
            "us_per_reset_given_probe_probe_cell": stat(times["reset_given_and_probes"]),
            "clear_over_solve_median": round(float(np.median(times["clear"]) / np.median(times["solve_same_updates"])), 3),
            "ms_per_solve_goal_poses_call": stat(whole), "reachable_share": round(float(out.reachable.mean()), 4),
            "free_share": round(float(out.free.mean()), 4), "pushed_share": round(float(out.pushed.mean()), 4)}


def _ik_oriented(a, solver, q0, targets, obstacles, R, K, per, prm) -> dict:
    """ik --orientation full|axis: the same queries with an orientation goal — axis: approach from above; full: the tool's z axis
    straight down and its x axis along the world's (the quaternion (1, 0, 0, 0)) — solved once for the converged and free shares,
    then the pose launch timed beside the positional launch in this process, the two alternating launch by launch."""
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd.environment.kinematic import orientation_goal
    kw = dict(orientations=[1.0, 0.0, 0.0, 0.0]) if a.orientation == "full" else dict(approach_directions=[0.0, 0.0, -1.0])
    out = solver.solve(q0, targets, obstacles, restarts=R, iterations=K, **kw)
    og = orientation_goal(len(q0), tolerance=1e-3, **kw)      # the last chunk's queries and goals are still in the buffers
    pose = solver.pose_params(og)
    times = {"positional": [], "pose": []}
    for i in range(2 * (a.launches + 2)):
        which = "pose" if i % 2 else "positional"
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        if which == "pose":
            solver.launch(per, R, prm, 1e-3, 0.0, solve_only=True, mode=og.mode, pose=pose)
        else:
            solver.launch(per, R, prm, 1e-3, 0.0, solve_only=True)
        t1.record()
        t1.synchronize()
        if i >= 4:
            times[which].append(1e3 * t0.elapsed_time(t1))
    stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1)}      # noqa: E731
    return {"kind": a.orientation, "iterations": K, "us_per_ik_solve_pose_launch": stat(times["pose"]),
            "us_per_ik_solve_launch_alternating": stat(times["positional"]),
            "pose_over_positional_median": round(float(np.median(times["pose"]) / np.median(times["positional"])), 3),
            "converged_share": round(float(out.reachable.mean()), 4), "free_share": round(float(out.free.mean()), 4),
            "median_angle_residual_of_converged": float(np.median(out.angle_residual[out.reachable])) if out.reachable.any() else None}


def paths(a):
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver, JointPathChecker
    from robotic_manipulator_rloa_amd.environment.kinematic import path_vias
    from robotic_manipulator_rloa_amd.environment.urdf_chain import compile_chain, load_urdf
    N, C, S, n = (2048 if a.envs == 64 else a.envs), 16, 256, a.joints
    launches = min(a.launches, 50)
    a.workcell = True
    urdf = os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf)
    init = ([0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0] + [0.0] * n)[:n]
    model = compile_chain(load_urdf(urdf), n - 1, list(range(n)), [n], init, [0.1] * n, 0.03, consider_autocollision=True, **_workcell(a))
    lib, dev, stream = _lib.load(), torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    lo = np.array([j.lower if j.limited else -np.pi for j in model.joints])
    hi = np.array([j.upper if j.limited else np.pi for j in model.joints])
    q_start, q_goal = np.tile(np.float32(init), (N, 1)), rng.uniform(lo, hi, (N, n)).astype(np.float32)
    obstacles = (np.array([0.35, 0.2, 0.45]) + rng.uniform(-0.2, 0.2, (N, 3))).astype(np.float32)
    checker = JointPathChecker(model, 0.06, certify=bool(a.certify))
    checker.load(q_start, q_goal, obstacles, path_vias(model, q_start, q_goal, C, 0))
    if a.certify:
        return _paths_certified(a, checker, model, N, C, S, launches, init, rng, urdf)
    if a.roadmap:
        return _paths_roadmap(a, checker, model, N, C, S, launches, init, rng, urdf, q_start, q_goal, obstacles)
    fused = []
    for i in range(launches + 2):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        checker.launch(N, C, S, 0.0)
        t1.record()
        t1.synchronize()
        if i >= 2:
            fused.append(1e3 * t0.elapsed_time(t1))
    # the composition, over the very poses the fused launch forms
    E, chunk = N * C * S, 1 << 20
    poses = torch.empty(E, n, device=dev)
    _lib.check(lib.naf_chain_path_check(checker._chain_env, checker.q_start.data_ptr(), checker.q_goal.data_ptr(), checker.vias.data_ptr(),
                                        checker.obstacles.data_ptr(), 0.06, N, C, S, 0.0, checker.out.data_ptr(), poses.data_ptr(), stream),
               "path_check")
    scene = torch.zeros(E, 6, device=dev)
    scene[:, 3:] = checker.obstacles[:N].repeat_interleave(C * S, dim=0)
    st = torch.zeros(chunk, lib.naf_chain_env_state_floats(checker._chain_env), device=dev)
    obs, probe, cell = torch.zeros(chunk, 2 * n + 9, device=dev), torch.zeros(E, 5, device=dev), torch.zeros(E, device=dev)
    composed = []
    for i in range(max(2, launches // 5) + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for first in range(0, E, chunk):
            e = min(chunk, E - first)
            _lib.check(lib.naf_chain_env_reset_given(checker._chain_env, st.data_ptr(), obs.data_ptr(), e, poses[first:].data_ptr(),
                                                     scene[first:].data_ptr(), 0.06, stream), "reset_given")
            _lib.check(lib.naf_chain_env_probe(checker._chain_env, st.data_ptr(), probe[first:].data_ptr(), e, stream), "probe")
            _lib.check(lib.naf_chain_env_probe_cell(checker._chain_env, st.data_ptr(), cell[first:].data_ptr(), e, stream), "probe_cell")
        t1.record()
        t1.synchronize()
        if i >= 1:
            composed.append(1e3 * t0.elapsed_time(t1))
    rec = checker.out[:N * C]
    mins = torch.stack([probe[:, 3].view(N * C, S).min(dim=1).values, probe[:, 4].view(N * C, S).min(dim=1).values,
                        cell.view(N * C, S).min(dim=1).values], dim=1)
    gap = float((rec[:, :3] - mins).abs().max())
    floats = lambda *ts: int(sum(t.numel() for t in ts) * 4)      # noqa: E731
    fused_bytes = floats(checker.q_start[:N], checker.q_goal[:N], checker.obstacles[:N], checker.vias[:N * C], checker.out[:N * C])
    composed_bytes = floats(poses, scene, st, obs, probe, cell)
    del poses, scene, st, obs, probe, cell
    # the README's question: can the goal be driven to? 2000 targets around the nominal one
    M = 2000
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.25, 0.25, (M, 3))
    start, obstacle = np.tile(init, (M, 1)), np.tile([0.35, 0.2, 0.45], (M, 1))
    goal = GoalPoseSolver(model, 0.06).solve(start, targets, obstacle)
    ok = goal.free
    found = checker.check(start[ok], goal.joint_positions[ok], obstacle[ok], candidates=C, resolution=0.02)
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")}
            for name, v in usage.items() if "chain_path_" in name}
    print(json.dumps({"arm": os.path.basename(urdf), "queries": N, "candidates": C, "samples": S, "self_pairs": len(model.self_pairs),
                      "workcell_pairs": len(model.cell_pairs), "boxes": bool(a.boxes),
                      "us_per_path_check_launch": {"median": round(float(np.median(fused)), 1), "min": round(float(np.min(fused)), 1)},
                      "us_per_reset_given_probe_probe_cell_over_all_poses": {"median": round(float(np.median(composed)), 1),
                                                                            "min": round(float(np.min(composed)), 1)},
                      "bytes_fused": fused_bytes, "bytes_composed": composed_bytes, "largest_difference_of_the_minima": gap,
                      "blocked_candidates_share": round(float((rec[:, 4] > 0).float().mean()), 4),
                      "targets": M, "free_goal_poses": int(ok.sum()),
                      "outcome_shares_among_free_goals": {k: round(float(np.mean(found.outcome == k)), 4)
                                                          for k in ("straight", "via", "blocked", "start", "goal")},
                      "median_samples": int(np.median(found.samples)), "largest_sample_step": round(float(found.sample_step.max()), 5),
                      "kernel_registers": regs}))


def _paths_certified(a, checker, model, N, C, S, launches, init, rng, urdf):
    import time
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    times = {"check": [], "certify": []}
    for i in range(launches + 2):                              # alternating, so that both see the same clocks
        for name, launch in (("check", checker.launch), ("certify", checker.launch_certify)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            launch(N, C, S, 0.0)
            t1.record()
            t1.synchronize()
            if i >= 2:
                times[name].append(1e3 * t0.elapsed_time(t1))
    rec, plain = checker.out_cert[:N * C], checker.out[:N * C]
    gap = float((rec[:, :3] - plain[:, :3]).nan_to_num(posinf=0.0).abs().max())
    M = 2000
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.25, 0.25, (M, 3))
    start, obstacle = np.tile(init, (M, 1)), np.tile([0.35, 0.2, 0.45], (M, 1))
    goal = GoalPoseSolver(model, 0.06).solve(start, targets, obstacle)
    ok = goal.free
    torch.cuda.synchronize()
    t = time.perf_counter()
    found = checker.check(start[ok], goal.joint_positions[ok], obstacle[ok], candidates=C, resolution=0.02)
    seconds = time.perf_counter() - t
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")}
            for name, v in usage.items() if "chain_path_" in name and "ChainCert" in name}
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"arm": os.path.basename(urdf), "queries": N, "candidates": C, "samples": S, "self_pairs": len(model.self_pairs),
                      "workcell_pairs": len(model.cell_pairs), "boxes": bool(a.boxes),
                      "us_per_path_check_launch": {"median": round(med["check"], 1), "min": round(float(np.min(times["check"])), 1)},
                      "us_per_path_certify_launch": {"median": round(med["certify"], 1), "min": round(float(np.min(times["certify"])), 1)},
                      "certify_over_check": round(med["certify"] / med["check"], 3), "largest_difference_of_the_minima": gap,
                      "free_candidates_share": round(float((rec[:, 4] == 0).float().mean()), 4),
                      "certified_candidates_share": round(float((rec[:, 11] == -1).float().mean()), 4),
                      "targets": M, "free_goal_poses": int(ok.sum()),
                      "outcome_shares_among_free_goals": {k: round(float(np.mean(found.outcome == k)), 4)
                                                          for k in ("straight", "via", "sampled", "blocked", "start", "goal")},
                      "refinements": {str(k): int(v) for k, v in zip(*np.unique(found.refinements, return_counts=True))},
                      "samples": {str(k): int(v) for k, v in zip(*np.unique(found.samples, return_counts=True))},
                      "seconds_all_rounds": round(seconds, 3), "kernel_registers": regs}))


def _paths_roadmap(a, checker, model, N, C, S, launches, init, rng, urdf, q_start, q_goal, obstacles):
    import time
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    from robotic_manipulator_rloa_amd.environment.kinematic import roadmap_edges, roadmap_milestones, roadmap_nodes
    M, V = a.roadmap, a.roadmap + 2
    edges = roadmap_edges(V)
    E = len(edges)
    n = max(1, min(N, N * C // E))                             # roadmaps whose edges are about as many workgroups as the N C paths
    nodes = roadmap_nodes(q_start, q_goal, roadmap_milestones(model, q_start, q_goal, M, 0))[:n]
    checker.load_edges(nodes, edges, obstacles[:n])
    times = {"check": [], "edges": []}
    for i in range(launches + 2):                              # alternating, so that both see the same clocks
        for name, launch in (("check", lambda: checker.launch(N, C, S, 0.0)), ("edges", lambda: checker.launch_edges(n, V, E, S, 0.0))):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            launch()
            t1.record()
            t1.synchronize()
            if i >= 2:
                times[name].append(1e3 * t0.elapsed_time(t1))
    rec = checker.edge_out[:n * E]
    T = 2000
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.25, 0.25, (T, 3))
    start, obstacle = np.tile(init, (T, 1)), np.tile([0.35, 0.2, 0.45], (T, 1))
    goal = GoalPoseSolver(model, 0.06).solve(start, targets, obstacle)
    ok = goal.free
    found, seconds = {}, {}
    for name, kw in (("one_via", {}), ("roadmap", {"roadmap": M})) + ((("shortcut", {"roadmap": M, "shortcut": a.shortcut}),)
                                                                     if a.shortcut else ()):
        torch.cuda.synchronize()
        t = time.perf_counter()
        found[name] = checker.check(start[ok], goal.joint_positions[ok], obstacle[ok], candidates=C, resolution=0.02, **kw)
        seconds[name] = round(time.perf_counter() - t, 3)
    kinds = ("straight", "via", "roadmap", "blocked", "start", "goal")
    with_map = found["roadmap"]
    rescued = with_map.outcome == "roadmap"
    shortcut = _shortcut_report(a, model, found, rescued, targets[ok], obstacle[ok]) if a.shortcut else None
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")}
            for name, v in usage.items() if "chain_edge_" in name}
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"arm": os.path.basename(urdf), "queries": N, "candidates": C, "samples": S, "self_pairs": len(model.self_pairs),
                      "workcell_pairs": len(model.cell_pairs), "boxes": bool(a.boxes), "milestones": M, "roadmaps": n, "edges": E,
                      "us_per_path_check_launch": {"median": round(med["check"], 1), "min": round(float(np.min(times["check"])), 1)},
                      "us_per_edge_check_launch": {"median": round(med["edges"], 1), "min": round(float(np.min(times["edges"])), 1)},
                      "ns_per_sample": {"path_check": round(1e3 * med["check"] / (N * C * S), 4),
                                        "edge_check": round(1e3 * med["edges"] / (n * E * S), 4)},
                      "free_edges_share": round(float((rec[:, 4] == 0).float().mean()), 4),
                      "targets": T, "free_goal_poses": int(ok.sum()),
                      "outcome_shares_among_free_goals": {name: {k: round(float(np.mean(p.outcome == k)), 4) for k in kinds}
                                                          for name, p in found.items()},
                      "blocked_without": int(np.sum(found["one_via"].outcome == "blocked")), "rescued": int(rescued.sum()),
                      "node_counts": {str(k): int(v) for k, v in zip(*np.unique(with_map.n_nodes[rescued], return_counts=True))},
                      "median_length_over_straight": (round(float(np.median(with_map.length[rescued] / with_map.straight_length[rescued])), 3)
                                                      if rescued.any() else None),
                      "roadmap_samples": {str(k): int(v) for k, v in zip(*np.unique(with_map.samples[rescued], return_counts=True))},
                      "edge_launches": checker.edge_launches - (launches + 2), "seconds": seconds, "shortcut": shortcut,
                      "kernel_registers": regs}))


def _shortcut_report(a, model, found, rescued, targets, obstacles):
    """--shortcut W: the 'roadmap' polylines before and after the shortcut round — length over the straight line, node counts,
    ticks at speed 1 — and how their demonstrations along all legs (demonstration_plan_legs, frames = 400) end"""
    import numpy as np
    from robotic_manipulator_rloa_amd.chain_tools import DemonstrationWriter
    from robotic_manipulator_rloa_amd.environment.kinematic import demonstration_plan_legs
    writer = DemonstrationWriter(model, 0.06)
    out = {"nodes": a.shortcut, "roadmap_queries": int(rescued.sum()),
           "shortened": int(np.sum(found["shortcut"].length[rescued] < found["roadmap"].length[rescued]))}
    for name in ("roadmap", "shortcut"):
        p = found[name]
        ratio = (p.length / p.straight_length)[rescued]
        plan = demonstration_plan_legs(p.nodes[rescued], p.n_nodes[rescued], 1.0, 400)
        demos = writer.write(plan, targets[rescued], obstacles[rescued], keep_contact=True)
        out[name] = {"median_length_over_straight": round(float(np.median(ratio)), 3), "max_length_over_straight": round(float(ratio.max()), 3),
                     "node_counts": {str(k): int(v) for k, v in zip(*np.unique(p.n_nodes[rescued], return_counts=True))},
                     "median_planned_ticks": int(np.median(demos.planned_ticks)),
                     "planned_ticks_within_400": int(np.sum(demos.planned_ticks <= 400)),
                     "demonstration_outcomes": {str(k): int(v) for k, v in zip(*np.unique(demos.outcome, return_counts=True))}}
    out["legs_launches"] = writer.legs_launches
    return out


def demo(a):
    """the one naf_chain_demo_rows launch (N x T rows) against the composed form: T x naf_chain_env_step at E = N, the actions
    already on the device, between device events"""
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_tools import DemonstrationWriter
    from robotic_manipulator_rloa_amd.environment.kinematic import demo_actions, demonstration_plan
    from robotic_manipulator_rloa_amd.environment.urdf_chain import compile_chain, load_urdf
    N, T, n = (2048 if a.envs == 64 else a.envs), 400, a.joints
    launches = min(a.launches, 30)
    a.workcell = True
    urdf = os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf)
    init = ([0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0] + [0.0] * n)[:n]
    model = compile_chain(load_urdf(urdf), n - 1, list(range(n)), [n], init, [0.1] * n, 0.03, consider_autocollision=True, **_workcell(a))
    lib, dev, stream = _lib.load(), torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    lo = np.array([j.lower if j.limited else -np.pi for j in model.joints])
    hi = np.array([j.upper if j.limited else np.pi for j in model.joints])
    # paths of T ticks or more at speed 1, so that every demonstration has T rows to write unless an outcome ends it
    q_start = np.tile(np.float32(init), (N, 1))
    q_goal = np.clip(q_start + rng.choice([-1.0, 1.0], (N, n)) * rng.uniform(0.6, 1.0, (N, n)) * (T / 240.0), lo, hi).astype(np.float32)
    via = (0.5 * (q_start + q_goal) + rng.uniform(-0.2, 0.2, (N, n))).astype(np.float32)
    targets = np.tile(np.float32([0.0, 0.0, 5.0]), (N, 1))
    obstacles = (np.array([0.35, 0.2, 0.45]) + rng.uniform(-0.2, 0.2, (N, 3))).astype(np.float32)
    plan = demonstration_plan(q_start, via, q_goal, 1.0, T)
    writer = DemonstrationWriter(model, 0.06, chunk=N * T)
    writer.load(plan, targets, obstacles, slice(0, N))
    if a.ticks:
        return _demo_ticks(a, writer, plan, targets, obstacles, N, T, launches, urdf, model)
    if a.legs:
        return _demo_legs(a, writer, plan, targets, obstacles, N, T, launches, urdf, model)
    fused = []
    for i in range(launches + 2):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        writer.launch(N, T)
        t1.record()
        t1.synchronize()
        if i >= 2:
            fused.append(1e3 * t0.elapsed_time(t1))
    rec = writer.records[:N].cpu().numpy()
    h = writer._chain_env
    S = 2 * n + 9
    rf = lib.naf_replay_row_floats(S, n)
    act = torch.from_numpy(np.ascontiguousarray(demo_actions(plan, T).transpose(1, 0, 2), np.float32)).to(dev)
    scene = torch.from_numpy(np.concatenate([targets, obstacles], axis=1)).to(dev)
    st, obs = torch.zeros(N, lib.naf_chain_env_state_floats(h), device=dev), torch.zeros(N, S, device=dev)
    rows = torch.zeros(T, N, rf, device=dev)
    composed = []
    for i in range(max(2, launches // 5) + 1):
        _lib.check(lib.naf_chain_env_reset_given(h, st.data_ptr(), obs.data_ptr(), N, writer.q_start.data_ptr(), scene.data_ptr(), 0.06,
                                                 stream), "reset_given")
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for t in range(T):
            _lib.check(lib.naf_chain_env_step(h, st.data_ptr(), act[t].data_ptr(), rows[t].data_ptr(), obs.data_ptr(), N, 0, None, 0, None,
                                              0, stream), "step")
        t1.record()
        t1.synchronize()
        if i >= 1:
            composed.append(1e3 * t0.elapsed_time(t1))
    # the first rows of both forms: the same positions and actions to the bit
    first = torch.equal(writer.rows[:N * T].view(N, T, rf)[:, 0, :n], rows[0, :, :n])
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")}
            for name, v in usage.items() if "chain_demo_" in name}
    f_med, c_med = float(np.median(fused)), float(np.median(composed))
    print(json.dumps({"arm": os.path.basename(urdf), "demonstrations": N, "ticks": T, "self_pairs": len(model.self_pairs),
                      "workcell_pairs": len(model.cell_pairs), "boxes": bool(a.boxes),
                      "us_per_demo_rows_launch": {"median": round(f_med, 1), "min": round(float(np.min(fused)), 1)},
                      "us_per_composed_steps": {"median": round(c_med, 1), "min": round(float(np.min(composed)), 1)},
                      "composed_over_fused": round(c_med / f_med, 3), "mean_valid_rows": round(float(rec[:, 0].mean()), 1),
                      "end_code_shares": {str(k): round(float(np.mean(rec[:, 1] == k)), 4) for k in range(6)},
                      "first_rows_bit_equal": bool(first), "kernel_registers": regs}))


def _demo_legs(a, writer, plan, targets, obstacles, N, T, launches, urdf, model):
    """--legs K: naf_chain_demo_rows_legs beside naf_chain_demo_rows, alternating in one process, on the same two-leg plans — the
    legs launch takes them split into K legs of the same actions (each leg of the plan cut into near-equal pieces), so that both
    write the same rows"""
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    K = a.legs
    ticks, acts = np.zeros((N, K), np.int32), np.zeros((N, K) + plan.leg_actions.shape[2:], np.float32)
    for n in range(N):
        col = 0
        for leg, parts in ((0, max(1, K // 2)), (1, K - max(1, K // 2))):
            total = int(plan.n_ticks[n, leg])
            parts = min(parts, total)
            for k in range(parts):
                ticks[n, col], acts[n, col] = total * (k + 1) // parts - total * k // parts, plan.leg_actions[n, leg]
                col += 1
    assert K >= 2 and np.array_equal(ticks.sum(axis=1), plan.n_ticks.sum(axis=1))
    two_rows = writer.rows
    legs_rows, legs_records, two_records = torch.zeros_like(two_rows), torch.zeros_like(writer.records), writer.records
    writer.load_legs(plan._replace(n_ticks=ticks, leg_actions=acts), targets, obstacles, slice(0, N))

    def launch_legs():
        writer.rows, writer.records = legs_rows, legs_records
        writer.launch_legs(N, K, T)
        writer.rows, writer.records = two_rows, two_records

    times = {"two_legs": [], "legs": []}
    for i in range(launches + 2):                              # alternating, so that both see the same clocks
        for name, launch in (("two_legs", lambda: writer.launch(N, T)), ("legs", launch_legs)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            launch()
            t1.record()
            t1.synchronize()
            if i >= 2:
                times[name].append(1e3 * t0.elapsed_time(t1))
    rec = two_records[:N].cpu().numpy()
    live = (torch.arange(T, device=two_rows.device)[None, :] < two_records[:N, 0].long()[:, None]).reshape(-1)
    same = torch.equal(two_rows[:N * T][live], legs_rows[:N * T][live]) and torch.equal(two_records[:N], legs_records[:N])
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")}
            for name, v in usage.items() if "chain_demo_" in name}
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"arm": os.path.basename(urdf), "demonstrations": N, "ticks": T, "legs": K, "self_pairs": len(model.self_pairs),
                      "workcell_pairs": len(model.cell_pairs), "boxes": bool(a.boxes),
                      "us_per_demo_rows_launch": {"median": round(med["two_legs"], 1), "min": round(float(np.min(times["two_legs"])), 1)},
                      "us_per_demo_rows_legs_launch": {"median": round(med["legs"], 1), "min": round(float(np.min(times["legs"])), 1)},
                      "legs_over_two_legs": round(med["legs"] / med["two_legs"], 3), "mean_valid_rows": round(float(rec[:, 0].mean()), 1),
                      "valid_rows_and_records_bit_equal": bool(same), "kernel_registers": regs}))


def _demo_ticks(a, writer, plan, targets, obstacles, N, T, launches, urdf, model):
    """--ticks: naf_chain_demo_rows_ticks beside naf_chain_demo_rows_legs, alternating in one process, on the same actions — the
    two-leg plans split into K legs (--legs K, default 5) for the legs launch, and demo_actions of that plan as the tick table —
    so that both write the same rows; and the whole writer call of either plan, upload and download included"""
    import time
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.environment.tick_demo import tick_plan_of
    K = a.legs or 5
    ticks, acts = np.zeros((N, K), np.int32), np.zeros((N, K) + plan.leg_actions.shape[2:], np.float32)
    for n in range(N):
        col = 0
        for leg, parts in ((0, max(1, K // 2)), (1, K - max(1, K // 2))):
            total = int(plan.n_ticks[n, leg])
            parts = min(parts, total)
            for k in range(parts):
                ticks[n, col], acts[n, col] = total * (k + 1) // parts - total * k // parts, plan.leg_actions[n, leg]
                col += 1
    legs_plan = plan._replace(n_ticks=ticks, leg_actions=acts)
    tick_plan = tick_plan_of(legs_plan, T)
    legs_rows, legs_records = writer.rows, writer.records
    tick_rows, tick_records = torch.zeros_like(legs_rows), torch.zeros_like(legs_records)
    writer.load_legs(legs_plan, targets, obstacles, slice(0, N))
    writer.load_ticks(tick_plan, targets, obstacles, slice(0, N))

    def launch_ticks():
        writer.rows, writer.records = tick_rows, tick_records
        writer.launch_ticks(N, T)
        writer.rows, writer.records = legs_rows, legs_records

    times = {"legs": [], "ticks": []}
    for i in range(launches + 2):                              # alternating, so that both see the same clocks
        for name, launch in (("legs", lambda: writer.launch_legs(N, K, T)), ("ticks", launch_ticks)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            launch()
            t1.record()
            t1.synchronize()
            if i >= 2:
                times[name].append(1e3 * t0.elapsed_time(t1))
    rec = legs_records[:N].cpu().numpy()
    live = (torch.arange(T, device=legs_rows.device)[None, :] < legs_records[:N, 0].long()[:, None]).reshape(-1)
    same = torch.equal(legs_rows[:N * T][live], tick_rows[:N * T][live]) and torch.equal(legs_records[:N], tick_records[:N])
    calls = {"legs": [], "ticks": []}
    for i in range(5):
        for name, p in (("legs", legs_plan), ("ticks", tick_plan)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            writer.write(p, targets, obstacles)
            torch.cuda.synchronize()
            if i >= 1:
                calls[name].append(1e3 * (time.perf_counter() - t0))
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")}
            for name, v in usage.items() if "chain_demo_ticks" in name or "chain_demo_legs" in name}
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"arm": os.path.basename(urdf), "demonstrations": N, "ticks": T, "legs": K, "self_pairs": len(model.self_pairs),
                      "workcell_pairs": len(model.cell_pairs), "boxes": bool(a.boxes),
                      "us_per_demo_rows_legs_launch": {"median": round(med["legs"], 1), "min": round(float(np.min(times["legs"])), 1)},
                      "us_per_demo_rows_ticks_launch": {"median": round(med["ticks"], 1), "min": round(float(np.min(times["ticks"])), 1)},
                      "ticks_over_legs": round(med["ticks"] / med["legs"], 3), "mean_valid_rows": round(float(rec[:, 0].mean()), 1),
                      "table_upload_mb": round(N * T * model.A * 4 / 1e6, 1),
                      "ms_per_writer_call": {k: round(float(np.median(v)), 2) for k, v in calls.items()},
                      "valid_rows_and_records_bit_equal": bool(same), "kernel_registers": regs}))


def edgecert(a):
    import time
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_certify import PolylineCertifier
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver, JointPathChecker
    from robotic_manipulator_rloa_amd.environment.kinematic import roadmap_edges, roadmap_milestones, roadmap_nodes
    from robotic_manipulator_rloa_amd.environment.urdf_chain import compile_chain, load_urdf
    n_joints, S, M, W = a.joints, 256, a.roadmap or 14, a.shortcut or 16
    V, n = M + 2, 273
    launches = min(a.launches, 50)
    a.workcell = True
    urdf = os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf)
    init = ([0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0] + [0.0] * n_joints)[:n_joints]
    model = compile_chain(load_urdf(urdf), n_joints - 1, list(range(n_joints)), [n_joints], init, [0.1] * n_joints, 0.03,
                          consider_autocollision=True, **_workcell(a))
    rng = np.random.default_rng(5)
    lo = np.array([j.lower if j.limited else -np.pi for j in model.joints])
    hi = np.array([j.upper if j.limited else np.pi for j in model.joints])
    q_start, q_goal = np.tile(np.float32(init), (n, 1)), rng.uniform(lo, hi, (n, n_joints)).astype(np.float32)
    obstacles = (np.array([0.35, 0.2, 0.45]) + rng.uniform(-0.2, 0.2, (n, 3))).astype(np.float32)
    nodes = roadmap_nodes(q_start, q_goal, roadmap_milestones(model, q_start, q_goal, M, 0))
    checker, certifier = JointPathChecker(model, 0.06), PolylineCertifier(model, 0.06)
    shapes = {"roadmaps": roadmap_edges(V), "polylines": np.stack([np.arange(V - 1), np.arange(1, V)], axis=1).astype(np.int32)}
    timing = {}
    for shape, edges in shapes.items():
        E = len(edges)
        checker.load_edges(nodes, edges, obstacles)
        certifier.edge_records(nodes, edges, obstacles, S, 0.0)              # (uploads, and one unmeasured launch)
        times = {"check": [], "certify": []}
        for i in range(launches + 2):                          # alternating, so that both see the same clocks
            for name, launch in (("check", lambda: checker.launch_edges(n, V, E, S, 0.0)), ("certify", lambda: certifier.launch(n, V, E, S, 0.0))):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                launch()
                t1.record()
                t1.synchronize()
                if i >= 2:
                    times[name].append(1e3 * t0.elapsed_time(t1))
        rec, plain = certifier.out[:n * E], checker.edge_out[:n * E]
        med = {k: float(np.median(v)) for k, v in times.items()}
        timing[shape] = {"items": n, "edges": E, "samples": S,
                         "us_per_edge_check_launch": {"median": round(med["check"], 1), "min": round(float(np.min(times["check"])), 1)},
                         "us_per_edge_certify_launch": {"median": round(med["certify"], 1), "min": round(float(np.min(times["certify"])), 1)},
                         "certify_over_check": round(med["certify"] / med["check"], 3),
                         "largest_difference_of_the_minima": float((rec[:, :3] - plain[:, :3]).nan_to_num(posinf=0.0).abs().max()),
                         "free_edges_share": round(float((rec[:, 4] == 0).float().mean()), 4),
                         "certified_edges_share": round(float((rec[:, 11] == -1).float().mean()), 4)}
    # the README's polylines: 2000 targets around the nominal one, the 'roadmap' answers without and with the shortcut round
    T = 2000
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.25, 0.25, (T, 3))
    start, obstacle = np.tile(init, (T, 1)), np.tile([0.35, 0.2, 0.45], (T, 1))
    goal = GoalPoseSolver(model, 0.06).solve(start, targets, obstacle)
    ok = goal.free
    census = {}
    for name, kw in (("roadmap", {"roadmap": M}), ("shortcut", {"roadmap": M, "shortcut": W})):
        found = checker.check(start[ok], goal.joint_positions[ok], obstacle[ok], candidates=16, resolution=0.02, **kw)
        rescued = found.outcome == "roadmap"
        census[name] = {"roadmap_queries": int(rescued.sum())}
        for label, margin in (("margin_0", 0.0), ("margin_2e-4_A_reach", 2e-4 * model.A * model.reach)):
            before = certifier.launches
            torch.cuda.synchronize()
            t = time.perf_counter()
            cert = certifier.certify(found, obstacle[ok], margin, 0.02)
            seconds = time.perf_counter() - t
            count = lambda x: {str(k): int(v) for k, v in zip(*np.unique(x, return_counts=True))}      # noqa: E731
            census[name][label] = {"margin": round(float(margin), 6), "roadmap_outcomes": count(cert.outcome[rescued]),
                                   "roadmap_refinements": count(cert.refinements[rescued]), "all_outcomes": count(cert.outcome),
                                   "all_refinements": count(cert.refinements), "launches": certifier.launches - before,
                                   "seconds": round(seconds, 3)}
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")}
            for name, v in usage.items() if "chain_edge_" in name and "ChainCert" in name}
    print(json.dumps({"arm": os.path.basename(urdf), "self_pairs": len(model.self_pairs), "workcell_pairs": len(model.cell_pairs),
                      "boxes": bool(a.boxes), "milestones": M, "shortcut_nodes": W, "launch": timing, "targets": T,
                      "free_goal_poses": int(ok.sum()), "polylines": census, "kernel_registers": regs}))


def line(a):
    import time
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import ManipulatorFramework, _lib
    from robotic_manipulator_rloa_amd.environment.line_moves import HOLD_FULL, HOLD_POSITION, line_constants
    N, W, U, n = (2048 if a.envs == 64 else a.envs), 32, 4, a.joints
    launches = min(a.launches, 50)
    urdf = os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf)
    init = ([0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0] + [0.0] * n)[:n]
    f = ManipulatorFramework()
    old = os.getcwd()
    os.chdir(tempfile.mkdtemp(prefix="naf_line_"))
    try:
        f.initialize_kinematic_environment(urdf, n - 1, [n], list(range(n)), [0.45, 0.3, 0.6], [0.35, 0.2, 0.45], init, [0.1] * n,
                                           link_radius=0.03, obstacle_radius=0.06, consider_autocollision=True, **_workcell(a))
    finally:
        os.chdir(old)
    model = f.env.model
    rng = np.random.default_rng(5)
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.15, 0.15, (N, 3))
    goal = f.solve_goal_poses(targets, approach_directions=[0, 0, -1], iterations=64)
    q = goal.joint_positions[goal.reachable]
    q = q[np.arange(N) % len(q)]                              # N start poses: the reachable ones, in turn
    disp = np.tile(np.float32([0.0, 0.0, 0.08]), (N, 1))
    whole = []
    for i in range(launches + 2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        moves = f.plan_linear_moves(q, disp, waypoints=W, updates=U)
        if i >= 2:
            whole.append(1e3 * (time.perf_counter() - t))
    tracker, solver = f.arm_planner.tools["line_moves"][1], f.arm_planner.tools["goal_poses"][1]
    c = line_constants(model)
    prm, pose = tracker.params(c, [0.0, 0.0, 1.0], [1.0, 0.0, 0.0])
    tracker.load(q[:tracker.chunk], disp[:tracker.chunk])
    per = min(N, tracker.chunk, solver.chunk)
    # the yardsticks' queries: the same start poses, one candidate each, W U iterations, the goal the tracker holds
    R_ee, ee = f.env.end_effector_frame(q[:per].astype(np.float64))
    solver.load(q[:per], ee + disp[:per], np.tile([0.35, 0.2, 0.45], (per, 1)), np.zeros((per, 1, model.A), np.float32))
    if solver.goals is None:
        solver.goals, solver.angle, solver.merit = solver._zeros(solver.chunk, 9), solver._zeros(solver.chunk), solver._zeros(solver.chunk)
    solver.goals.view(-1)[:per * 9].copy_(torch.from_numpy(np.ascontiguousarray(R_ee.reshape(-1), np.float32)))
    ik_prm = _lib.IkParams(W * U, c["lam2"], c["e_max"], c["dq_max"])
    out = {}
    for name, mode in (("full", HOLD_FULL), ("position", HOLD_POSITION)):
        times = {"track": [], "solve": []}
        for i in range(2 * (launches + 2)):
            which = "track" if i % 2 else "solve"
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            if which == "track":
                tracker.launch(per, mode, W, U, prm, pose)
            elif mode == HOLD_FULL:
                solver.launch(per, 1, ik_prm, 1e-3, 0.0, solve_only=True, mode=0, pose=pose)
            else:
                solver.launch(per, 1, ik_prm, 1e-3, 0.0, solve_only=True)
            t1.record()
            t1.synchronize()
            if i >= 4:
                times[which].append(1e3 * t0.elapsed_time(t1))
        stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1)}      # noqa: E731
        out[name] = {"us_per_line_track_launch": stat(times["track"]),
                     "us_per_ik_solve_pose_launch" if mode == HOLD_FULL else "us_per_ik_solve_launch": stat(times["solve"]),
                     "track_over_solve_median": round(float(np.median(times["track"]) / np.median(times["solve"])), 3)}
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {k: v.get(k) for k in ("vgprs", "sgprs", "scratch_bytes_per_lane", "occupancy")} for name, v in usage.items()
            if "chain_line_track" in name}
    print(json.dumps({"arm": os.path.basename(urdf), "lines": N, "lines_per_launch": per, "waypoints": W, "updates": U,
                      "yardstick_iterations": W * U, **out,
                      "ms_per_plan_linear_moves_call_host_clock": {"median": round(float(np.median(whole)), 2),
                                                                   "min": round(float(np.min(whole)), 2)},
                      "outcomes": {k: int(v) for k, v in zip(*np.unique(moves.outcome, return_counts=True))},
                      "samples_per_leg": int(moves.samples[0]), "worst_position_error": float(np.nanmax(moves.position_error)),
                      "worst_angle_error": float(np.nanmax(moves.angle_error)), "worst_line_deviation": float(np.nanmax(moves.line_deviation)),
                      "start_poses_reachable_of": [int(goal.reachable.sum()), N], "kernel_registers": regs}))


def traj(a):
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_certify import PolylineCertifier
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver, JointPathChecker
    from robotic_manipulator_rloa_amd.chain_traj import TrajectoryChecker
    from robotic_manipulator_rloa_amd.environment.edge_certificate import polyline_nodes
    from robotic_manipulator_rloa_amd.environment.kinematic import roadmap_edges
    from robotic_manipulator_rloa_amd.environment.trajectory import DeviceSchedule, blend_schedule, device_schedule
    from robotic_manipulator_rloa_amd.environment.urdf_chain import compile_chain, load_urdf
    n_joints, M, W, N, dt = a.joints, a.roadmap or 14, a.shortcut or 16, (2048 if a.envs == 64 else a.envs), 1.0 / 240.0
    launches = min(a.launches, 50)
    a.workcell = True
    urdf = os.path.abspath(a.urdf) if os.path.isabs(a.urdf) else os.path.join(ROOT, a.urdf)
    init = ([0.0, 0.6, 0.0, -1.2, 0.0, 0.8, 0.0] + [0.0] * n_joints)[:n_joints]
    model = compile_chain(load_urdf(urdf), n_joints - 1, list(range(n_joints)), [n_joints], init, [0.1] * n_joints, 0.03,
                          consider_autocollision=True, **_workcell(a))
    rng = np.random.default_rng(5)
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.25, 0.25, (N, 3))
    start, obstacle = np.tile(init, (N, 1)), np.tile([0.35, 0.2, 0.45], (N, 1))
    goal = GoalPoseSolver(model, 0.06).solve(start, targets, obstacle)
    ok = goal.free
    checker, certifier, tool = JointPathChecker(model, 0.06), PolylineCertifier(model, 0.06), TrajectoryChecker(model, 0.06)
    found = checker.check(start[ok], goal.joint_positions[ok], obstacle[ok], candidates=16, resolution=0.02, roadmap=M, shortcut=W)
    ob = obstacle[ok]
    vmax, amax = np.full(n_joints, 1.0), np.full(n_joints, 4.0)
    # the launch, beside the edge launch over the same number of walked poses
    nodes, count = polyline_nodes(found)
    has = np.flatnonzero(count >= 2)
    sched = [blend_schedule(nodes[q, :count[q]].astype(np.float32).astype(np.float64), vmax, amax) for q in has]
    ds = device_schedule(sched, dt)
    S = -(-int(ds.n_samples.max()) // 256) * 256              # a multiple of 256: E edges of 256 samples walk the same S poses
    per = min(len(has), tool.chunk // S)
    part = DeviceSchedule(*(x[:per] for x in ds[:5]), ds.dt)
    E, V = S // 256, nodes.shape[1] if nodes.shape[1] * (nodes.shape[1] - 1) // 2 >= S // 256 else 16
    edge_nodes = np.zeros((per, V, n_joints), np.float32)
    edge_nodes[:, :part.nodes.shape[1]] = part.nodes
    edge_nodes[:, part.nodes.shape[1]:] = part.nodes[:, -1:]
    edges = roadmap_edges(V)[:E]
    checker.load_edges(edge_nodes, edges, ob[has[:per]])
    timing = {}
    for certify in ((False, True) if a.certify else (False,)):
        tool.records(part, ob[has[:per]], S, 0.0, certify, False)            # (uploads, and one unmeasured launch)
        if certify:
            certifier.edge_records(edge_nodes, edges, ob[has[:per]], 256, 0.0)
        edge_launch = (lambda: certifier.launch(per, V, E, 256, 0.0)) if certify else (lambda: checker.launch_edges(per, V, E, 256, 0.0))
        times = {"edge": [], "traj": []}
        for i in range(launches + 2):                          # alternating, so that both see the same clocks
            for name, launch in (("edge", edge_launch), ("traj", lambda: tool.launch(per, part.nodes.shape[1], S, ds.dt, 0.0, certify, False))):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                launch()
                t1.record()
                t1.synchronize()
                if i >= 2:
                    times[name].append(1e3 * t0.elapsed_time(t1))
        stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1)}      # noqa: E731
        timing["certify" if certify else "check"] = {
            "us_per_edge_launch": stat(times["edge"]), "us_per_traj_launch": stat(times["traj"]),
            "traj_over_edge_median": round(float(np.median(times["traj"]) / np.median(times["edge"])), 3)}
    # the shares: the trajectories of the free polylines, and of the certified ones
    count_of = lambda x: {str(k): int(v) for k, v in zip(*np.unique(x, return_counts=True))}      # noqa: E731
    import time
    before, whole = tool.launches, []
    for i in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        plain = tool.plan(found, ob, vmax, amax, dt, False, 0.0, positions=False)
        whole.append(1e3 * (time.perf_counter() - t))
    per_call = (tool.launches - before) // 5
    margin = 2e-4 * model.A * model.reach
    cert_poly = certifier.certify(found, ob, margin, 0.02)
    cert_traj = tool.plan(found, ob, vmax, amax, dt, True, margin, positions=False)
    ratio = (plain.duration / plain.rest_to_rest_duration)[plain.outcome != "none"]
    usage = json.load(open(_lib.USAGE_PATH)) if os.path.exists(_lib.USAGE_PATH) else {}
    regs = {name: {q: v.get(q) for q in ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")}
            for name, v in usage.items() if "chain_traj_" in name}
    print(json.dumps({"arm": os.path.basename(urdf), "self_pairs": len(model.self_pairs), "workcell_pairs": len(model.cell_pairs),
                      "boxes": bool(a.boxes), "targets": N, "free_goal_poses": int(ok.sum()), "polylines": int(len(has)),
                      "path_outcomes": count_of(found.outcome), "vmax": 1.0, "amax": 4.0, "dt": dt,
                      "launch": {"trajectories": per, "ticks": S, "edges_of_256_samples": E, "walked_poses": per * S, **timing},
                      "ms_per_plan_call_host_clock": {"median": round(float(np.median(whole[1:])), 1), "launches": per_call},
                      "trajectories_of_free_polylines": count_of(plain.outcome[plain.outcome != "none"]),
                      "margin": round(float(margin), 6), "polyline_certificates": count_of(cert_poly.outcome),
                      "trajectories_of_certified_polylines": count_of(cert_traj.outcome[cert_poly.outcome == "certified"]),
                      "duration_over_rest_to_rest": {"median": round(float(np.median(ratio)), 3), "min": round(float(ratio.min()), 3),
                                                     "max": round(float(ratio.max()), 3)},
                      "ticks_per_trajectory": {"median": int(np.median(plain.n_samples[plain.n_samples > 0])), "max": int(plain.n_samples.max())},
                      "corner_deviation_rad": {"median": round(float(np.nanmedian(plain.corner_deviation)), 4),
                                               "max": round(float(np.nanmax(plain.corner_deviation)), 4)},
                      "kernel_registers": regs}))


def kernels(a):
    import numpy as np
    import torch
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.environment.urdf_chain import compile_chain, load_urdf
    lib = _lib.load()
    dev = torch.device("cuda:0")
    E, stream = a.envs, torch.cuda.current_stream().cuda_stream
    for name, n in (("standin8", 8), ("long32", 32)):
        model = compile_chain(load_urdf(os.path.join(URDF, name + ".urdf")), n - 1, list(range(n)), [], None, [0.1] * n, 0.03,
                              consider_autocollision=a.autocollision)
        blob = np.ascontiguousarray(model.pack())
        h = ctypes.c_void_p()
        _lib.check(lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(h)), "create")
        S = 2 * n + 9
        st = torch.zeros(E, lib.naf_chain_env_state_floats(h), device=dev)
        obs, act = torch.zeros(E, S, device=dev), torch.randn(E, n, device=dev)
        rows = torch.zeros(E, lib.naf_replay_row_floats(S, n), device=dev)
        scene = (ctypes.c_float * 8)(0.4, 0.85, 0.71, 0.45, 0.55, 0.55, 0.0, 0.06)
        _lib.check(lib.naf_chain_env_reset(h, st.data_ptr(), obs.data_ptr(), E, scene, 5, 0, stream), "reset")
        for _ in range(a.launches):
            _lib.check(lib.naf_chain_env_step(h, st.data_ptr(), act.data_ptr(), rows.data_ptr(), obs.data_ptr(), E, 5, None, 0, None, 0,
                                              stream), "step")
        torch.cuda.synchronize()
        lib.naf_chain_env_destroy(h)
    n, S = 8, 25
    st = torch.zeros(E, lib.naf_synth_env_state_floats(n), device=dev)
    obs, act, rows = torch.zeros(E, S, device=dev), torch.randn(E, n, device=dev), torch.zeros(E, 64, device=dev)
    _lib.check(lib.naf_synth_env_reset(st.data_ptr(), obs.data_ptr(), E, n, 5, 0, None, 0, stream), "reset")
    for _ in range(a.launches):
        _lib.check(lib.naf_synth_env_step(st.data_ptr(), act.data_ptr(), rows.data_ptr(), obs.data_ptr(), E, n, 5, None, 0, None, 0,
                                          stream), "step")
    torch.cuda.synchronize()
    print(json.dumps({"launches_each": a.launches, "envs": E, "autocollision": a.autocollision}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rate", "kernels", "step", "rollout", "gather", "ik", "path", "demo", "edgecert", "line", "traj"])
    ap.add_argument("--urdf", default=os.path.join("tests", "golden", "urdf", "iiwa_like7.urdf"))
    ap.add_argument("--joints", type=int, default=7)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--standin-only", action="store_true")
    ap.add_argument("--autocollision", action="store_true")
    ap.add_argument("--workcell", action="store_true", help="step / rollout: a floor and two spheres in the chain model")
    ap.add_argument("--boxes", action="store_true", help="step / rollout / path, with --workcell: three boxes beside the floor and the spheres")
    ap.add_argument("--certify", action="store_true", help="path: time naf_chain_path_certify beside naf_chain_path_check, and certify the README's paths; traj: also time the certifying launches")
    ap.add_argument("--roadmap", type=int, default=0, metavar="M",
                    help="path: time naf_chain_edge_check beside naf_chain_path_check, and answer the README's paths with M milestones")
    ap.add_argument("--shortcut", type=int, default=0, metavar="W",
                    help="path, with --roadmap: answer the README's paths again with a shortcut round over W nodes, and demonstrate them")
    ap.add_argument("--legs", type=int, default=0, metavar="K",
                    help="demo: time naf_chain_demo_rows_legs, the same plans split into K legs, beside naf_chain_demo_rows")
    ap.add_argument("--ticks", action="store_true",
                    help="demo: time naf_chain_demo_rows_ticks beside naf_chain_demo_rows_legs on the same actions, and the whole writer call")
    ap.add_argument("--orientation", choices=["full", "axis"], default=None,
                    help="ik: also solve the section's queries with an orientation goal and time naf_chain_ik_solve_pose beside naf_chain_ik_solve")
    ap.add_argument("--avoid-contact", action="store_true",
                    help="ik: also solve with the null-space push and time naf_chain_ik_clear beside naf_chain_ik_solve and the probes")
    ap.add_argument("--trajectory", action="store_true", help="rollout: record the joint values of every frame")
    ap.add_argument("--arm", default="", help="rate: a fixture arm of tests/golden/urdf by name, --joints its joint count")
    ap.add_argument("--target-range", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--obstacle-range", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--hindsight", type=float, default=None, help="rate, gather: the share of rows replayed under a hindsight goal")
    ap.add_argument("--horizon", type=int, default=None, help="rate, gather: hindsight_horizon (rate: max_frames; gather: 400)")
    a = ap.parse_args()
    if a.roadmap and a.certify and a.what not in ("edgecert", "traj"):
        ap.error("--roadmap and --certify are two measurements: roadmap edges are checked at their samples only")
    if a.shortcut and not a.roadmap and a.what not in ("edgecert", "traj"):
        ap.error("--shortcut shortens roadmap paths: it needs --roadmap M")
    if a.legs and not 2 <= a.legs <= 63:
        ap.error("--legs K splits two-leg plans into K legs, 2 .. 63")
    {"rate": rate, "kernels": kernels, "step": step, "rollout": rollout, "gather": gather, "ik": ik, "path": paths, "demo": demo,
     "edgecert": edgecert, "line": line, "traj": traj}[a.what](a)


if __name__ == "__main__":
    main()
