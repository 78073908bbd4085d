"""Time-parameterised trajectories along joint-space polylines, and their collision check at a controller's ticks,
stated once in float64 as environment/kinematic.py states the rest: the schedule of a polyline under velocity and acceleration
limits (blend_schedule), the law of linear segments with parabolic blends (trajectory_law), what the device is given of it in
float32 (device_schedule), the one table of half-steps a trajectory has (trajectory_half_steps), the record of a checked trajectory
(check_trajectory), and the ONE control flow that the device and the twin run alike (plan_trajectories; _TwinTrajectories is its
twin backend). numpy only.

THE LAW. A polyline P_0 .. P_K, K >= 1, consecutive equal nodes merged. Leg k = 1 .. K runs P_{k-1} -> P_k in T_k at the velocity
v_k = (P_k - P_{k-1}) / T_k; v_0 = v_{K+1} = 0. Node k has the nominal time t_k = tau_0 / 2 + T_1 + .. + T_k and a blend of
duration tau_k centred on it, inside which the acceleration is a_k = (v_{k+1} - v_k) / tau_k (0 where tau_k = 0). Two virtual legs
complete it: leg 0, P_0 -> P_0 over [0, t_0], and leg K + 1, P_K -> P_K over [t_K, D], D = t_K + tau_K / 2. Blends never overlap:
(tau_{k-1} + tau_k) / 2 <= T_k. At a time t inside leg j (the largest j whose start — 0 for j = 0, t_{j-1} otherwise — is <= t),
with s = t - start:
    h0 = max(0, tau_{j-1} / 2 - s)        h1 = max(0, (t - t_j) + tau_j / 2)
    q(t)  = P_{j-1} + v_j s + 1/2 a_{j-1} h0^2 + 1/2 a_j h1^2
    q'(t) = v_j - a_{j-1} h0 + a_j h1
(P_{-1} = P_0; tau and a are 0 outside 0 .. K). q(0) = P_0 and q(t) = P_K for t >= D, exactly; the trajectory starts and ends at
rest; an interior node is passed at the joint-space distance |v_{k+1} - v_k| tau_k / 8, not through.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from .urdf_chain import ChainModel

TRAJ_NODES_MAX = 64                   # V: nodes per trajectory on the device, 2 .. 64 (K <= 63 legs)
TRAJ_SAMPLES_MIN, TRAJ_SAMPLES_MAX = 64, 8192      # S of a launch: a multiple of 64
TRAJ_CHUNK = 1 << 23                  # samples per chunk (queries x S, whole queries), on the device and through the twin alike
TRAJ_ROUNDS = 16                      # rounds of the leg-wise stretch before the uniform one
TRAJ_NUDGE = 1e-6                     # the uniform stretch is nudged up by this share when it fires
TRAJ_FLOATS, TRAJ_CERT_FLOATS = 8, 12               # NAF_CHAIN_EDGE_FLOATS, NAF_CHAIN_EDGE_CERT_FLOATS
TRAJECTORY_OUTCOMES = ("free", "certified", "sampled", "blocked", "none")


def merge_nodes(poly) -> np.ndarray:
    """poly[n][A] without the nodes that equal their predecessor; at least one node stays"""
    poly = np.asarray(poly, np.float64)
    keep = np.ones(len(poly), bool)
    keep[1:] = np.any(poly[1:] != poly[:-1], axis=1)
    return poly[keep]


def _blend_times(P, T, amax):
    """(v[K + 2][A] with v_0 = v_{K+1} = 0, tau[K + 1]) of the leg durations T[K]"""
    v = np.zeros((len(T) + 2, P.shape[1]))
    v[1:-1] = (P[1:] - P[:-1]) / T[:, None]
    return v, np.max(np.abs(v[1:] - v[:-1]) / amax, axis=1)


def blend_schedule(poly, vmax, amax) -> dict:
    """The schedule of ONE polyline poly[n][A] (merge_nodes is applied) under vmax[A], amax[A] > 0, in float64: a dict of nodes
    [K + 1][A], leg_times T[K], blend_times tau[K + 1], node_times t[K + 1], duration D, rounds (how many leg-wise rounds stretched a
    leg) and scaled (the uniform factor, 1.0 where it did not fire). T_k starts at max_m |dP_km| / vmax_m; up to TRAJ_ROUNDS times,
    with tau_k = max_m |v_{k+1,m} - v_{k,m}| / amax_m and rho_k = (tau_{k-1} + tau_k) / (2 T_k), every leg with rho_k > 1 takes
    T_k <- T_k sqrt(rho_k), all from the same tau; then ONE uniform scaling of all T_k by sqrt(max(1, max rho)), nudged up by
    TRAJ_NUDGE where it is above 1 — scaling by f divides every rho by f^2, so the blends of the result never overlap. A polyline
    of one node has K = 0, D = 0."""
    P = merge_nodes(poly)
    vmax, amax = np.asarray(vmax, np.float64), np.asarray(amax, np.float64)
    K = len(P) - 1
    if K == 0:
        z = np.zeros(0)
        return dict(nodes=P, leg_times=z, blend_times=np.zeros(1), node_times=np.zeros(1), duration=0.0, rounds=0, scaled=1.0)
    T = np.max(np.abs(P[1:] - P[:-1]) / vmax, axis=1)
    rounds = 0
    for _ in range(TRAJ_ROUNDS):
        _, tau = _blend_times(P, T, amax)
        rho = (tau[:-1] + tau[1:]) / (2.0 * T)
        if not np.any(rho > 1.0):
            break
        T = np.where(rho > 1.0, T * np.sqrt(np.maximum(rho, 1.0)), T)
        rounds += 1
    _, tau = _blend_times(P, T, amax)
    worst = float(np.max((tau[:-1] + tau[1:]) / (2.0 * T)))
    scaled = 1.0
    if worst > 1.0:
        scaled = math.sqrt(worst) * (1.0 + TRAJ_NUDGE)
        T = T * scaled
        _, tau = _blend_times(P, T, amax)
    t = 0.5 * tau[0] + np.concatenate([[0.0], np.cumsum(T)])
    return dict(nodes=P, leg_times=T, blend_times=tau, node_times=t, duration=float(t[-1] + 0.5 * tau[-1]), rounds=rounds, scaled=scaled)


def rest_to_rest_duration(poly, vmax, amax) -> float:
    """the duration of the polyline with a stop at every corner: per leg the slowest joint's trapezoid (or triangle) under its own
    two limits, the legs summed"""
    P = merge_nodes(poly)
    d = np.abs(P[1:] - P[:-1])
    vmax, amax = np.asarray(vmax, np.float64), np.asarray(amax, np.float64)
    trapezoid = d / vmax + vmax / amax
    triangle = 2.0 * np.sqrt(d / amax)
    return float(np.sum(np.max(np.where(d >= vmax * vmax / amax, trapezoid, triangle), axis=1))) if len(d) else 0.0


def trajectory_law(nodes, n_nodes, node_times, blend_times, inv_leg_times, t, derivative: bool = False) -> np.ndarray:
    """q(t) (or q'(t)) of the law above, in float64, for batched schedules: nodes[..., V, A], n_nodes[...] (K + 1),
    node_times[..., V], blend_times[..., V], inv_leg_times[..., V] (1 / T_k at k, 0 at k = 0), t[..., S] -> [..., S, A]. Entries
    behind n_nodes are not read. This is the twin of the device's evaluation: the same selections and the same sums, in float64 on
    whatever values it is given (a float32 schedule's, for the device's twin)."""
    P = np.asarray(nodes, np.float64)
    n = np.asarray(n_nodes, np.int64)[..., None]
    tk, tau, iT = (np.asarray(x, np.float64) for x in (node_times, blend_times, inv_leg_times))
    t = np.asarray(t, np.float64)
    V = P.shape[-2]
    K = n - 1
    live = np.arange(V) < n[..., None]                                      # [..., 1, V]
    j = np.sum(live & (tk[..., None, :] <= t[..., None]), axis=-1)          # [..., S], 0 .. K + 1

    def pick(x, k, ok):
        """x[..., V] at index k[..., S] where ok, else 0"""
        got = np.take_along_axis(np.broadcast_to(x[..., None, :], k.shape + (V,)), np.clip(k, 0, V - 1)[..., None], axis=-1)[..., 0]
        return np.where(ok, got, 0.0)

    def node(k):
        k = np.clip(k, 0, K)
        return np.take_along_axis(np.broadcast_to(P[..., None, :, :], k.shape + P.shape[-2:]), k[..., None, None], axis=-2)[..., 0, :]

    start = pick(tk, j - 1, j >= 1)
    s = t - start
    tau_p, tau_n = pick(tau, j - 1, j >= 1), pick(tau, j, j <= K)
    h0 = np.maximum(0.0, 0.5 * tau_p - s)
    h1 = np.where(j <= K, np.maximum(0.0, (t - pick(tk, j, j <= K)) + 0.5 * tau_n), 0.0)
    with np.errstate(divide="ignore"):
        wp, wn = np.where(tau_p > 0.0, 1.0 / tau_p, 0.0), np.where(tau_n > 0.0, 1.0 / tau_n, 0.0)
    pm2, pm1, p0, p1 = node(j - 2), node(j - 1), node(j), node(j + 1)
    v_prev = (pm1 - pm2) * pick(iT, j - 1, (j - 1 >= 1))[..., None]
    v = (p0 - pm1) * pick(iT, j, (j >= 1) & (j <= K))[..., None]
    v_next = (p1 - p0) * pick(iT, j + 1, j + 1 <= K)[..., None]
    if derivative:
        return v - (v - v_prev) * (wp * h0)[..., None] + (v_next - v) * (wn * h1)[..., None]
    c0, c1 = 0.5 * h0 * h0 * wp, 0.5 * h1 * h1 * wn
    return pm1 + v * s[..., None] + c0[..., None] * (v - v_prev) + c1[..., None] * (v_next - v)


def law_of(schedule: dict, t, derivative: bool = False) -> np.ndarray:
    """trajectory_law on one blend_schedule's float64 values: t[S] -> [S, A]"""
    P, T = schedule["nodes"], schedule["leg_times"]
    with np.errstate(divide="ignore"):
        iT = np.concatenate([[0.0], 1.0 / T])
    return trajectory_law(P, len(P), schedule["node_times"], schedule["blend_times"], iT, np.asarray(t, np.float64), derivative)


def _round_up32(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    y = x.astype(np.float32)
    return np.where(y.astype(np.float64) < x, np.nextafter(y, np.float32(np.inf)), y).astype(np.float32)


class DeviceSchedule(NamedTuple):
    """What a launch is given, float32 (int32 counts): the values the twin evaluates the law on in float64"""
    nodes: np.ndarray               # [N][V][A]: P_k, P_K repeated behind a query's last node
    n_nodes: np.ndarray             # [N] int32: K + 1
    times: np.ndarray               # [N][V][3]: (t_k, tau_k, 1 / T_k), the last 0 at k = 0; zeros behind a query's last node
    vpeak: np.ndarray               # [N][A]: max_k |v_km| of THESE float32 values, formed in float64 and rounded up
    n_samples: np.ndarray           # [N] int32: S_n = ceil(D_n / dt) + 1, D_n = t_K + tau_K / 2 of these float32 values
    dt: float                       # as float32 holds it


def device_schedule(schedules, dt: float, V: Optional[int] = None) -> DeviceSchedule:
    """The float32 schedule of a list of blend_schedule dicts. t_0 is tau_0 / 2 OF THE FLOAT32 tau_0 (exact in float32), so that
    q(0) = P_0 exactly for the device and its twin."""
    N, A = len(schedules), schedules[0]["nodes"].shape[1]
    V = max(2, max(len(s["nodes"]) for s in schedules)) if V is None else int(V)
    nodes, times = np.zeros((N, V, A), np.float32), np.zeros((N, V, 3), np.float32)
    count, n_samples, vpeak = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros((N, A), np.float32)
    dt32 = float(np.float32(dt))
    for n, s in enumerate(schedules):
        k = len(s["nodes"])
        count[n] = k
        nodes[n, :k], nodes[n, k:] = s["nodes"], s["nodes"][-1]
        times[n, :k, 1] = s["blend_times"]
        times[n, :k, 0] = s["node_times"]
        times[n, 0, 0] = np.float32(0.5) * times[n, 0, 1]
        if k > 1:
            times[n, 1:k, 2] = 1.0 / s["leg_times"]
            v = (nodes[n, 1:k].astype(np.float64) - nodes[n, :k - 1].astype(np.float64)) * times[n, 1:k, 2].astype(np.float64)[:, None]
            vpeak[n] = _round_up32(np.abs(v).max(axis=0))
        D = float(times[n, k - 1, 0]) + 0.5 * float(times[n, k - 1, 1])
        n_samples[n] = int(math.ceil(D / dt32)) + 1
    return DeviceSchedule(nodes, count, times, vpeak, n_samples, dt32)


def sample_times(S: int, dt: float) -> np.ndarray:
    """[S] float64: t_i = (float)i dt as float32 forms it"""
    return (np.arange(S).astype(np.float32) * np.float32(dt)).astype(np.float64)


def trajectory_poses(ds: DeviceSchedule, S: int) -> np.ndarray:
    """[N][S][A] float64: the law at the S ticks, on the float32 schedule's values"""
    t = np.broadcast_to(sample_times(S, ds.dt), (len(ds.n_nodes), S))
    return trajectory_law(ds.nodes, ds.n_nodes, ds.times[..., 0], ds.times[..., 1], ds.times[..., 2], t)


def trajectory_half_steps(model: ChainModel, vpeak, dt: float, reach=None) -> np.ndarray:
    """[..., n_seg + P] float64: the ONE table of a trajectory. Between two ticks joint m moves at most vpeak_m dt, so over half a
    tick a point of capsule s travels at most beta[s] = 1/2 dt sum_m vpeak_m R[m][s]; entry n_seg + p, pair p = (s, t): the same sum
    over the joints between the two frames with R[m][t] — edge_half_steps' span rule."""
    from .kinematic import reach_table
    R = (reach_table(model) if reach is None else np.asarray(reach)).astype(np.float64)
    n_seg = len(model.segments)
    W = np.zeros((model.A, n_seg + len(model.self_pairs)))
    W[:, :n_seg] = R
    for p, (s, t) in enumerate(model.self_pairs):
        f_s, f_t = model.segments[s].frame, model.segments[t].frame
        W[f_s:f_t, n_seg + p] = R[f_s:f_t, t]
    return 0.5 * float(dt) * np.asarray(vpeak, np.float64) @ W


def check_trajectory(twin, ds: DeviceSchedule, obstacles, S: int, margin: float = 0.0, certify: bool = False, poses=None,
                     reach=None, guard: Optional[float] = None) -> np.ndarray:
    """[N][TRAJ_FLOATS or TRAJ_CERT_FLOATS] float64, the records of the trajectories of `ds` in the scenes obstacles[N][3] at S
    ticks: [0] [1] [2] the minima over the LIVE samples (i < S_n) of the obstacle clearance (its radius subtracted), the
    self-clearance and the workcell clearance | [3] the first blocked live sample, -1: none | [4] how many are blocked | [5] D in
    float32 | [6] max_m vpeak_m dt in float32, the bound on a joint's step between two ticks | [7] whether the last live sample is
    blocked | certify: [8] [9] [10] the minima over the live samples of (clearance - beta - guard) per kind, beta
    trajectory_half_steps' | [11] the first live sample one of whose slacks is < margin, -1: none. Samples i >= S_n count in
    nothing. COVERAGE: a pose between two ticks is within half a tick of the nearer one, over which no point of a tested capsule
    travels farther than its beta; so if every test at every live sample keeps margin + beta + guard, no pose of the trajectory is
    closer than margin. poses[N][S][A]: evaluate the clearances there (the tests' teacher forcing)."""
    from .kinematic import certificate_guard, path_slacks
    N = len(ds.n_nodes)
    ob = np.asarray(obstacles, np.float64).reshape(N, 3)
    q = trajectory_poses(ds, S) if poses is None else np.asarray(poses, np.float64)
    live = np.arange(S)[None, :] < ds.n_samples[:, None]
    clear = twin.clearance(q, ob[:, None, :]) - twin.obstacle_radius
    zero = np.zeros(clear.shape)
    m = np.stack([clear, twin.self_clearance(q) + zero, twin.cell_clearance(q) + zero], axis=-1)
    blocked = np.any(m < margin, axis=-1) & live
    out = np.empty((N, TRAJ_CERT_FLOATS if certify else TRAJ_FLOATS))
    out[:, :3] = np.where(live[..., None], m, np.inf).min(axis=1)
    out[:, 3] = np.where(blocked.any(axis=1), np.argmax(blocked, axis=1), -1)
    out[:, 4] = blocked.sum(axis=1)
    last = ds.times[np.arange(N), ds.n_nodes - 1]
    out[:, 5] = last[:, 0] + np.float32(0.5) * last[:, 1]
    out[:, 6] = (ds.vpeak * np.float32(ds.dt)).max(axis=1)
    out[:, 7] = blocked[np.arange(N), np.clip(ds.n_samples - 1, 0, S - 1)]
    if certify:
        guard = certificate_guard(twin.model) if guard is None else float(guard)
        beta = trajectory_half_steps(twin.model, ds.vpeak, ds.dt, reach)
        slack = path_slacks(twin, q, ob, (beta, beta, beta), guard)
        low = np.any(slack < margin, axis=-1) & live
        out[:, 8:11] = np.where(live[..., None], slack, np.inf).min(axis=1)
        out[:, 11] = np.where(low.any(axis=1), np.argmax(low, axis=1), -1)
    return out


class _TrajectoryFields(NamedTuple):
    outcome: np.ndarray                 # [N] str: 'free' | 'certified' | 'sampled' (free at the ticks, not certified; only with
                                        # certify) | 'blocked' (a tick is below the margin) | 'none' (the query has no path)
    duration: np.ndarray                # [N]: D; NaN for 'none'
    rest_to_rest_duration: np.ndarray   # [N]: the duration with a stop at every corner
    n_samples: np.ndarray               # [N] int: S_n, the ticks 0 .. S_n - 1; 0 for 'none'
    first_blocked: np.ndarray           # [N] int: the first blocked tick, -1: none
    first_blocked_time: np.ndarray      # [N]: its time; NaN where none
    min_clearance: np.ndarray           # [N]: least obstacle clearance over the ticks; NaN for 'none'
    min_self_clearance: np.ndarray      # [N]: ... self-clearance, +inf without pairs
    min_cell_clearance: np.ndarray      # [N]: ... workcell clearance, +inf without a workcell
    corner_deviation: np.ndarray        # [N]: the largest |v_{k+1} - v_k| tau_k / 8 over the interior nodes, max-norm
    peak_velocity: np.ndarray           # [N][A]: max_k |v_km|
    peak_acceleration: np.ndarray       # [N][A]: max_k |a_km|
    slack: Optional[np.ndarray]         # [N]: the least of the three slacks (certify only, else None)
    certified: Optional[np.ndarray]     # [N] bool (certify only, else None)
    leg_times: np.ndarray               # [N][Kmax]: T_k, NaN-padded
    blend_times: np.ndarray             # [N][Kmax + 1]: tau_k, NaN-padded
    positions: Optional[np.ndarray]     # [N][Smax][A]: the pose at every tick, NaN behind each query's own end; None if not asked
    nodes: np.ndarray                   # [N][Kmax + 1][A]: the merged polylines the schedule is of, NaN-padded
    n_nodes: np.ndarray                 # [N] int: K + 1; 0 for 'none'
    dt: float                           # the tick


class Trajectories(_TrajectoryFields):
    """What plan_trajectories says about N queries (ManipulatorFramework.plan_trajectories). The verdicts are about the capsule
    model and the law; a controller's tracking error is not in them."""
    __slots__ = ()

    def _law(self, times, derivative: bool) -> np.ndarray:
        t = np.asarray(times, np.float64)
        N = len(self.n_nodes)
        t = np.broadcast_to(t, (N,) + t.shape[-1:]) if t.ndim <= 1 or t.shape[0] != N else t
        fill = lambda x: np.where(np.isnan(x), 0.0, x)      # noqa: E731
        T, tau = fill(np.asarray(self.leg_times, np.float64)), fill(np.asarray(self.blend_times, np.float64))
        tk = 0.5 * tau[:, :1] + np.concatenate([np.zeros((N, 1)), np.cumsum(T, axis=1)], axis=1)
        with np.errstate(divide="ignore"):
            iT = np.concatenate([np.zeros((N, 1)), np.where(T > 0.0, 1.0 / T, 0.0)], axis=1)
        out = trajectory_law(fill(np.asarray(self.nodes, np.float64)), np.maximum(self.n_nodes, 1), tk, tau, iT, t, derivative)
        return np.where((np.asarray(self.n_nodes) >= 1)[:, None, None], out, np.nan)

    def at(self, times) -> np.ndarray:
        """[N][S][A]: q(t) of the float64 law at times[S] (for all queries) or times[N][S]; NaN for 'none'"""
        return self._law(np.atleast_1d(times), False)

    def velocities(self, times=None) -> np.ndarray:
        """[N][S][A]: q'(t) of the float64 law at the given times, by default at the ticks i dt, i < max n_samples"""
        if times is None:
            times = np.arange(max(int(np.max(self.n_samples)), 1) if len(self.n_samples) else 1) * float(self.dt)
        return self._law(np.atleast_1d(times), True)


def trajectory_chunks(n_samples, budget: int) -> list:
    """[(queries (an index array), S)]: the queries in the order of their S_n (the first of equals first), cut into chunks. A chunk's
    S is the largest S_n in it rounded up to a multiple of 64; a query joins the chunk in front of it as long as queries x S stays
    within `budget` samples and S stays within twice the chunk's first query's — a trajectory walks the whole S of its launch, its
    dead samples included, so a launch of mixed lengths would walk mostly dead ones. A chunk holds at least one query; a
    trajectory's result does not depend on its chunk."""
    up = lambda s: max(TRAJ_SAMPLES_MIN, -(-int(s) // 64) * 64)      # noqa: E731
    order = np.argsort(np.asarray(n_samples), kind="stable")
    out, first, N = [], 0, len(order)
    while first < N:
        n, S0 = 1, up(n_samples[order[first]])
        S = S0
        while first + n < N:
            S2 = up(n_samples[order[first + n]])
            if (n + 1) * S2 > budget or S2 > 2 * S0:
                break
            n, S = n + 1, S2
        out.append((order[first:first + n], S))
        first += n
    return out


def limits_of(name: str, value, A: int) -> np.ndarray:
    """a limit given as a scalar or [A], as [A] float64, positive and finite; ValueError otherwise"""
    try:
        v = np.array(value, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} is a positive number, or [{A}] of them") from None
    if isinstance(value, (bool, np.bool_)) or v.shape not in ((), (A,)):
        raise ValueError(f"{name} is a positive number, or [{A}] of them, one per joint: got shape {v.shape}")
    v = np.broadcast_to(v, (A,)).copy()
    if not np.all(np.isfinite(v) & (v > 0.0)):
        raise ValueError(f"{name} is positive and finite for every joint: got {v.tolist()}")
    return v


def plan_trajectories(backend, nodes, n_nodes, obstacles, vmax, amax, dt: float, certify: bool = False, margin: float = 0.0,
                      positions: bool = True, budget: int = TRAJ_CHUNK) -> Trajectories:
    """The ONE control flow of trajectories, run by the device (chain_traj.TrajectoryChecker) and by the twin (_TwinTrajectories)
    alike. nodes[N][Kmax][A], n_nodes[N] (edge_certificate.polyline_nodes'), obstacles[N][3], vmax[A], amax[A], dt. A query without
    a path (fewer than 1 node) is 'none' and is never passed to the backend. Every other query gets blend_schedule's schedule in
    float64, handed on as float32 (device_schedule); where an S_n exceeds TRAJ_SAMPLES_MAX the longest query is refused by name with the
    dt that fits. backend.records(ds, obstacles[n], S, margin, certify, positions) -> (records[n][8 | 12], poses[n][S][A] | None) checks one
    chunk (trajectory_chunks). 'blocked': a live tick is below the margin; with certify 'certified' iff [11] == -1, else 'sampled';
    without it 'free'."""
    nodes, count = np.asarray(nodes, np.float64), np.asarray(n_nodes, np.int64)
    N, A = len(count), nodes.shape[-1]
    ob = np.asarray(obstacles, np.float64).reshape(N, 3)
    dtype = backend.dtype
    has = np.flatnonzero(count >= 1)
    # (the nodes are taken as float32 holds them: the schedule is of the polyline the device is given)
    sched = [blend_schedule(nodes[q, :count[q]].astype(np.float32).astype(np.float64), vmax, amax) for q in has]
    Kmax = max([len(s["nodes"]) for s in sched] + [2])
    nan = lambda *shape: np.full((N,) + shape, np.nan, dtype)      # noqa: E731
    nan64 = lambda *shape: np.full((N,) + shape, np.nan)      # noqa: E731  (the schedule is the host's, float64 for either backend)
    out = dict(outcome=np.full(N, "none", "<U9"), duration=nan64(), rest_to_rest_duration=nan64(), n_samples=np.zeros(N, np.int64),
               first_blocked=np.full(N, -1, np.int64), first_blocked_time=nan64(), min_clearance=nan(), min_self_clearance=nan(),
               min_cell_clearance=nan(), corner_deviation=nan64(), peak_velocity=nan64(A), peak_acceleration=nan64(A),
               slack=nan() if certify else None, certified=np.zeros(N, bool) if certify else None, leg_times=nan64(Kmax - 1),
               blend_times=nan64(Kmax), positions=None, nodes=nan64(Kmax, A), n_nodes=np.zeros(N, np.int64), dt=float(dt))
    if not len(has):
        out["positions"] = np.full((N, 0, A), np.nan, dtype) if positions else None
        return Trajectories(**out)
    ds = device_schedule(sched, dt, Kmax)
    over = np.flatnonzero(ds.n_samples > TRAJ_SAMPLES_MAX)
    if len(over):
        i = int(np.argmax(ds.n_samples))                     # the longest of them: the dt that fits it fits every query
        q, D = int(has[i]), float(sched[i]["duration"])
        raise ValueError(f"plan_trajectories: query {q} lasts {D:.6g} s, {int(ds.n_samples[i])} ticks at dt={float(dt):.6g}: a "
                         f"trajectory holds at most {TRAJ_SAMPLES_MAX}; dt >= {D / (TRAJ_SAMPLES_MAX - 2):.6g} fits")
    for i, (q, s) in enumerate(zip(has, sched)):
        k, v = len(s["nodes"]), np.zeros((len(s["nodes"]) + 1, A))
        if k > 1:
            v[1:-1] = (s["nodes"][1:] - s["nodes"][:-1]) / s["leg_times"][:, None]
        dv = np.abs(v[1:] - v[:-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.where(s["blend_times"][:, None] > 0.0, dv / s["blend_times"][:, None], 0.0)
        out["duration"][q] = s["duration"]
        out["rest_to_rest_duration"][q] = rest_to_rest_duration(s["nodes"], vmax, amax)
        out["n_samples"][q], out["n_nodes"][q] = ds.n_samples[i], k
        out["corner_deviation"][q] = np.max(dv[1:-1].max(axis=1) * s["blend_times"][1:-1] / 8.0) if k > 2 else 0.0
        out["peak_velocity"][q], out["peak_acceleration"][q] = np.abs(v).max(axis=0), acc.max(axis=0)
        out["leg_times"][q, :k - 1], out["blend_times"][q, :k], out["nodes"][q, :k] = s["leg_times"], s["blend_times"], s["nodes"]
    records = np.empty((len(has), TRAJ_CERT_FLOATS if certify else TRAJ_FLOATS), dtype)
    Smax = int(ds.n_samples.max())
    if positions:
        out["positions"] = np.full((N, Smax, A), np.nan, dtype)
    for sl, S in trajectory_chunks(ds.n_samples, budget):
        part = DeviceSchedule(ds.nodes[sl], ds.n_nodes[sl], ds.times[sl], ds.vpeak[sl], ds.n_samples[sl], ds.dt)
        records[sl], poses = backend.records(part, ob[has[sl]], S, margin, certify, positions)
        if positions:
            for i, k in enumerate(sl):
                out["positions"][has[k], :ds.n_samples[k]] = poses[i, :ds.n_samples[k]]
    blocked = records[:, 4] > 0
    if certify:
        cert = ~blocked & (records[:, 11] == -1)
        out["outcome"][has] = np.where(blocked, "blocked", np.where(cert, "certified", "sampled"))
        out["certified"][has], out["slack"][has] = cert, records[:, 8:11].min(axis=1)
    else:
        out["outcome"][has] = np.where(blocked, "blocked", "free")
    out["first_blocked"][has] = records[:, 3].astype(np.int64)
    out["first_blocked_time"][has] = np.where(blocked, records[:, 3].astype(np.float64) * ds.dt, np.nan)
    out["min_clearance"][has], out["min_self_clearance"][has], out["min_cell_clearance"][has] = records[:, 0], records[:, 1], records[:, 2]
    return Trajectories(**out)


class _TwinTrajectories:
    """plan_trajectories' backend through the twin alone: the float64 law on the float32 schedule, the twin's clearances and
    path_slacks; a few trajectories at a time"""
    dtype = np.float64

    def __init__(self, twin):
        self.twin = twin
        self.reach = self.guard = None                        # formed on the first certifying call, as the device tool's are

    def records(self, ds: DeviceSchedule, obstacles, S: int, margin: float, certify: bool, positions: bool):
        if certify and self.reach is None:
            from .kinematic import certificate_guard, reach_table
            self.reach, self.guard = reach_table(self.twin.model), certificate_guard(self.twin.model)
        n = len(ds.n_nodes)
        out = np.empty((n, TRAJ_CERT_FLOATS if certify else TRAJ_FLOATS))
        poses = np.empty((n, S, ds.nodes.shape[-1])) if positions else None
        block = max(1, 65536 // S)
        for k in range(0, n, block):
            sl = slice(k, k + block)
            part = DeviceSchedule(ds.nodes[sl], ds.n_nodes[sl], ds.times[sl], ds.vpeak[sl], ds.n_samples[sl], ds.dt)
            q = trajectory_poses(part, S)
            out[sl] = check_trajectory(self.twin, part, obstacles[sl], S, margin, certify, q, self.reach, self.guard)
            if positions:
                poses[sl] = q
        return out, poses


def trajectories_host(twin, paths, obstacles, vmax, amax, dt: float, certify: bool = False, margin: float = 0.0,
                      positions: bool = True, chunk: Optional[int] = None) -> Trajectories:
    """plan_trajectories through the twin alone on the polylines of `paths` (edge_certificate.polyline_nodes), the obstacles rounded
    to float32 as the device is given them"""
    from .edge_certificate import polyline_nodes
    nodes, count = polyline_nodes(paths)
    ob = np.asarray(obstacles, np.float64).astype(np.float32).astype(np.float64).reshape(len(count), 3)
    return plan_trajectories(_TwinTrajectories(twin), nodes, count, ob, vmax, amax, dt, certify, float(np.float32(margin)), positions,
                             TRAJ_CHUNK if chunk is None else int(chunk))
