"""The scripted scenarios of fixture G9 (tests/golden/g9_env.npz): what the scripted simulator (tests/scripted_pybullet.py) answers,
frame by frame, and which Environment calls are recorded. Ours; make_golden.py --only g9 runs them through the unmodified reference.

Every rule case fills one frame; a step scenario shows four of them, one per tick, and probes every frame (the first frame is free
space), so each case is seen by step() and by get_reward / is_terminal_state with and without consider_autocollision.
"""
import numpy as np

OP_NONE, OP_PROBE, OP_STEP, OP_RESET = -1, 0, 1, 2
F, P = 5, 9                       # frames and operations of every scenario (padded)
NEVER = 10 ** 6

ROBOTS = {      # name: (joints, involved, fixed, end effector, a link outside `involved`)
    "kuka": (7, [0, 1, 2, 3, 4, 5], [6], 6, 6),
    "xarm6": (7, [1, 2, 3, 4, 5, 6], [0], 6, 0),
    "arm12": (12, [0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11], 11, 9),
}

T = 0.05
T_LO, T_HI = float(np.nextafter(T, 0.0)), float(np.nextafter(T, 1.0))
TINY = 5e-324                     # the float64 neighbours of 0.0 are +-TINY


def _cases(ee, outside):
    """(name, end-effector-target distance, {link: obstacle distance}, {(link, link): self distance}, everything else empty?)"""
    nan = float("nan")
    return [
        ("free", 0.31, {}, {}, False),
        ("target_at_threshold", T, {}, {}, False),
        ("target_below_threshold", T_LO, {}, {}, False),
        ("target_above_threshold", T_HI, {}, {}, False),
        ("obstacle_at_zero", 0.2, {2: 0.0}, {}, False),
        ("obstacle_below_zero", 0.2, {2: -TINY}, {}, False),
        ("obstacle_above_zero", 0.2, {2: TINY}, {}, False),
        ("obstacle_on_uninvolved_link", 0.4, {outside: -0.01}, {}, False),
        ("obstacle_on_inner_link", 0.4, {3: -0.02}, {}, False),
        ("reached_and_obstacle", 0.03, {3: -0.01}, {}, False),
        ("self_contact", 0.25, {}, {(0, 4): -0.001}, False),
        ("reached_and_self_contact", 0.02, {}, {(5, 1): -0.5}, False),
        ("nothing_within_range", nan, {}, {}, True),
        ("obstacle_and_self_contact", 0.6, {1: -0.3}, {(2, 5): -0.2}, False),
        ("self_at_zero", 0.7, {}, {(1, 3): 0.0}, False),
        ("self_below_zero", 0.7, {}, {(1, 3): -TINY}, False),
        ("target_beyond_range", 12.0, {}, {}, False),
        ("neighbours_overlap", 0.15, {}, {(2, 3): -0.1, (3, 2): -0.1, (4, 4): -1.0}, False),
        ("every_threshold_met", T, {ee: 0.0}, {(0, 2): 0.0}, False),
        ("obstacle_on_end_effector", 0.09, {ee: -0.004}, {}, False),
    ]


def _blank(name, robot, rng):
    n, involved, fixed, ee, _ = ROBOTS[robot]
    A = len(involved)
    sc = dict(name=name, robot=robot, n=n, ee=ee, involved=involved, fixed=fixed, max_force=200.0, init=None, var=None,
              target=rng.uniform(0.2, 0.9, 3).round(3), obstacle=rng.uniform(-0.6, 0.1, 3).round(3),
              switch=np.arange(1, F), joints=rng.uniform(-2.0, 2.0, (F, n, 2)).round(4), ee_pos=rng.uniform(-1.0, 1.0, (F, 3)).round(4),
              obstacle_d=np.empty((F, n)), target_d=np.empty((F, n)), self_d=np.empty((F, n, n)),
              ops=np.full((P, 1 + A), np.nan))
    sc["ops"][:, 0] = OP_NONE
    for f in range(F):
        _fill(sc, f, ("free", 0.31 + 0.1 * f, {}, {}, False))
    return sc


def _fill(sc, f, case):
    _, d_target, obstacle, selfd, empty = case
    n, ee = sc["n"], sc["ee"]
    link = np.arange(n)
    sc["obstacle_d"][f] = np.nan if empty else 0.5 + 0.01 * link
    sc["obstacle_d"][f, 1 % n] = np.nan                           # one empty answer in every frame
    sc["target_d"][f] = np.nan if empty else 0.01                 # every other link is well inside the threshold ...
    sc["target_d"][f, ee] = d_target                              # ... only the end effector's distance counts
    sc["self_d"][f] = np.nan if empty else 0.3
    sc["self_d"][f, 0, n - 1] = np.nan
    for j, d in obstacle.items():
        sc["obstacle_d"][f, j] = d
    for (i, j), d in selfd.items():
        sc["self_d"][f, i, j] = d


def scenarios():
    out = []
    for r, robot in enumerate(ROBOTS):
        n, involved, fixed, ee, outside = ROBOTS[robot]
        A = len(involved)
        rng = np.random.Generator(np.random.PCG64(900 + r))
        cases = _cases(ee, outside)
        for g in range(0, len(cases), F - 1):
            sc = _blank(f"{robot}/steps{g // (F - 1)}", robot, rng)
            sc["max_force"] = 200.0 if g == 0 else 75.5
            sc["cases"] = ["free"] + [c[0] for c in cases[g:g + F - 1]]
            sc["ops"][0, 0] = OP_PROBE
            for t, case in enumerate(cases[g:g + F - 1]):
                _fill(sc, t + 1, case)
                sc["ops"][1 + 2 * t, 0] = OP_STEP
                sc["ops"][1 + 2 * t, 1:] = rng.uniform(-1.0, 1.0, A).round(4)
                sc["ops"][2 + 2 * t, 0] = OP_PROBE
            out.append(sc)
        if robot == "xarm6":
            continue
        for k, (has_init, has_var) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            sc = _blank(f"{robot}/reset{k}", robot, rng)
            sc["cases"] = ["free"] * F
            sc["init"] = rng.uniform(-1.5, 1.5, n).round(3) if has_init else None
            sc["var"] = rng.uniform(0.05, 0.4, n).round(3) if has_var else None
            sc["switch"] = np.array([50, 51, NEVER, NEVER])
            sc["ops"][0, :2] = OP_RESET, 40 + k
            sc["ops"][1, 0] = OP_PROBE
            sc["ops"][2, 0] = OP_STEP
            sc["ops"][2, 1:] = rng.uniform(-1.0, 1.0, A).round(4)
            sc["ops"][3, 0] = OP_PROBE
            out.append(sc)
    return out


_STACKED = ("target", "obstacle", "switch", "joints", "ee_pos", "obstacle_d", "target_d", "self_d", "ops")


def pack(scs, records):
    """the arrays of g9_env.npz: per robot, the scenarios stacked along axis 0. records[k] = (states, numbers, log, base)."""
    out = {}
    for robot, (n, involved, fixed, ee, _) in ROBOTS.items():
        ks = [k for k, sc in enumerate(scs) if sc["robot"] == robot]
        out[f"{robot}/dims"] = np.array([n, ee])
        out[f"{robot}/involved"], out[f"{robot}/fixed"] = np.array(involved), np.array(fixed)
        out[f"{robot}/names"] = np.array([scs[k]["name"] for k in ks])
        out[f"{robot}/cases"] = np.array([scs[k]["cases"] for k in ks])
        out[f"{robot}/max_force"] = np.array([scs[k]["max_force"] for k in ks])
        for key in ("init", "var"):
            out[f"{robot}/{key}"] = np.array([np.full(n, np.nan) if scs[k][key] is None else scs[k][key] for k in ks])
        for key in _STACKED:
            out[f"{robot}/{key}"] = np.array([scs[k][key] for k in ks], float)
        out[f"{robot}/states"] = np.array([records[k][0] for k in ks])
        out[f"{robot}/numbers"] = np.array([records[k][1] for k in ks])
        calls = max(len(records[k][2]) for k in ks)
        log = np.full((len(ks), calls, 6), np.nan)
        for i, k in enumerate(ks):
            log[i, :len(records[k][2])] = records[k][2]
        out[f"{robot}/log"], out[f"{robot}/log_rows"] = log, np.array([len(records[k][2]) for k in ks])
        bases = max(len(records[k][3]) for k in ks)
        base = np.full((len(ks), bases, 7), np.nan)
        for i, k in enumerate(ks):
            base[i, :len(records[k][3])] = records[k][3]
        out[f"{robot}/base"] = base
    return out


def unpack(z):
    """the scenarios and their records back from g9_env.npz: [(scenario, (states, numbers, log, base))]"""
    out = []
    for robot in ROBOTS:
        n, ee = (int(v) for v in z[f"{robot}/dims"])
        for i, name in enumerate(z[f"{robot}/names"]):
            opt = lambda key: None if np.isnan(z[f"{robot}/{key}"][i]).all() else z[f"{robot}/{key}"][i]
            sc = dict(name=str(name), robot=robot, n=n, ee=ee, involved=[int(j) for j in z[f"{robot}/involved"]],
                      fixed=[int(j) for j in z[f"{robot}/fixed"]], max_force=float(z[f"{robot}/max_force"][i]),
                      init=opt("init"), var=opt("var"), cases=[str(c) for c in z[f"{robot}/cases"][i]])
            for key in _STACKED:
                sc[key] = z[f"{robot}/{key}"][i]
            rows = int(z[f"{robot}/log_rows"][i])
            base = z[f"{robot}/base"][i]
            rec = (z[f"{robot}/states"][i], z[f"{robot}/numbers"][i], z[f"{robot}/log"][i][:rows],
                   base[~np.isnan(base).any(axis=1)])
            out.append((sc, rec))
    return out
