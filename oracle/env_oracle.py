"""
oracle/env_oracle.py — TEST INFRASTRUCTURE ONLY. The reference environment's RULE, stated once in plain Python / numpy: what a set of
distances is worth and whether it ends the episode, how the state is laid out, and which motor commands a step sends in which order.

The reference computes all of this from PyBullet's answers (distances from getClosestPoints, joint and link states); the rule is
what it does with those numbers, and it runs without Bullet. tests/test_oracle_golden.py holds this file to tests/golden/g9_env.npz,
which tests/golden/make_golden.py --only g9 recorded from the unmodified reference's Environment under a scripted simulator; every
other statement of the rule in this repository (the PyBullet adapter, the synthetic and kinematic environments and their kernels,
the hindsight relabelling) is held to this file. Nothing under robotic_manipulator_rloa_amd/ imports it.

Line citations are to the reference checkout (JavierMtz5/robotic_manipulator_rloa), robotic_manipulator_rloa/environment/
environment.py unless another file is named.

`defect`: None, or one of DEFECTS — the rule wrong in one way. The tests use the mutants to show that their cases would notice.
"""
from __future__ import annotations

import numpy as np

TARGET_THRESHOLD = 0.05        # get_reward's and is_terminal_state's default (:311, :364)
OBSTACLE_THRESHOLD = 0.0       # (:311, :368)
REACHED_REWARD = 250           # an int (:367)
CONTACT_REWARD = -1000         # an int (:369)
MAX_DISTANCE = 10.0            # what an empty getClosestPoints answer counts as (utils/collision_detector.py:33, :56-57)
RESET_TICKS = 50               # (:300)
POSITION_CONTROL, VELOCITY_CONTROL = 2, 0          # pybullet's constants
CALL_MOTOR, CALL_TICK, CALL_BASE = 0, 1, 2          # rows of a call log: [kind, joint, mode, by, value, force], NaN: not given
BY_POSITION, BY_VELOCITY = 0, 1

DEFECTS = ("obstacle_before_target", "le_for_lt", "threshold_not_subtracted", "reward_sign", "self_without_flag",
           "self_ignored_with_flag", "done_without_reached", "target_obstacle_swapped", "joints_at_involved",
           "contact_on_involved_only")
#   obstacle_before_target     the reward asks for contact before it asks whether the target is reached
#   le_for_lt                  <= where the reference compares with <
#   threshold_not_subtracted   the shaped reward is -d instead of -(d - 0.05)
#   reward_sign                the shaped reward is +(d - 0.05)
#   self_without_flag          self-collision counts although consider_autocollision is off
#   self_ignored_with_flag     self-collision does not count although consider_autocollision is on
#   done_without_reached       reaching the target does not end the episode
#   target_obstacle_swapped    the state ends [.., obstacle, target]
#   joints_at_involved         the state's joint columns are read at the involved joints' indices
#   contact_on_involved_only   obstacle contact is looked for on the involved joints' links only


def distance_of(points, max_distance: float = MAX_DISTANCE) -> float:
    """One getClosestPoints answer as a distance: the smallest contact distance (field 8 of a record), max_distance for the empty
    answer (utils/collision_detector.py:56-59, :93-96)."""
    return max_distance if len(points) == 0 else float(min(pt[8] for pt in points))


def self_pairs(num_joints: int):
    """The (link, other link) pairs get_manipulator_collisions_with_itself asks about, in its order: every ordered pair except a
    link with itself and with its two neighbours (:401-410, utils/collision_detector.py:74-80)."""
    return [(i, j) for i in range(num_joints) for j in range(num_joints) if abs(i - j) > 1]


def _below(x, threshold, defect) -> bool:
    x = np.asarray(x, float)
    return bool((x <= threshold).any() if defect == "le_for_lt" else (x < threshold).any())


def rule(d_target, d_obstacle_links, self_distances, consider_autocollision: bool = False, defect=None, involved=None):
    """(reward, done) as get_reward(consider_autocollision) and is_terminal_state(consider_autocollision=...) return them.
    d_target: the end effector's distance to the target; d_obstacle_links: every link's distance to the obstacle;
    self_distances: the distances between the pairs of self_pairs (any shape; may be empty).
      reached  = d_target < 0.05                                                   (:364, :429)
      contact  = any link's obstacle distance < 0                                  (:368, :383-392)
      self     = consider_autocollision and any self distance < 0                  (:357-362, :336-341)
      reward   = 250 if reached, else -1000 if contact or self, else -1 * float(d_target - 0.05)      (:366-371)
      done     = 1 if contact, else 1 if reached, else 1 if self, else 0           (:326-343)
    The reward is the int 250 or -1000, or a float. step() asks both without the flag (:481-483).
    `involved` is read by the defect contact_on_involved_only alone."""
    assert defect is None or defect in DEFECTS
    d_target = float(d_target)
    d_obstacle_links = np.asarray(d_obstacle_links, float).reshape(-1)
    if defect == "contact_on_involved_only":
        d_obstacle_links = d_obstacle_links[list(involved)]
    flag = bool(consider_autocollision)
    if defect == "self_without_flag":
        flag = True
    if defect == "self_ignored_with_flag":
        flag = False
    self_hit = flag and _below(self_distances, 0.0, defect)
    reached = _below(d_target, TARGET_THRESHOLD, defect)
    contact = _below(d_obstacle_links, OBSTACLE_THRESHOLD, defect)
    if defect == "threshold_not_subtracted":
        shaped = -1 * float(d_target)
    elif defect == "reward_sign":
        shaped = float(d_target - TARGET_THRESHOLD)
    else:
        shaped = -1 * float(d_target - TARGET_THRESHOLD)
    if defect == "obstacle_before_target":
        reward = CONTACT_REWARD if (contact or self_hit) else (REACHED_REWARD if reached else shaped)
    else:
        reward = REACHED_REWARD if reached else (CONTACT_REWARD if (contact or self_hit) else shaped)
    ends = contact or self_hit or (reached and defect != "done_without_reached")
    return reward, 1 if ends else 0


def outcome(d_target, d_obstacle_links, self_distances, consider_autocollision: bool = False) -> str:
    """which branch of `rule` gave the reward: "reached", "contact" or "free" """
    reward, _ = rule(d_target, d_obstacle_links, self_distances, consider_autocollision)
    return "reached" if reward is REACHED_REWARD or reward == REACHED_REWARD else ("contact" if reward == CONTACT_REWARD else "free")


def state_of(joint_states, involved, ee, target, obstacle, defect=None) -> np.ndarray:
    """get_state (:440-451): [q, qdot, end effector, target, obstacle] in float64. joint_states[j] = (position, velocity) of joint
    j for every joint of the arm; the joints read are 0 .. len(involved) - 1, whatever `involved` holds (:442-444)."""
    assert defect is None or defect in DEFECTS
    joint_states = np.asarray(joint_states, float)
    read = list(involved) if defect == "joints_at_involved" else list(range(len(involved)))
    tail = (obstacle, target) if defect == "target_obstacle_swapped" else (target, obstacle)
    return np.hstack([joint_states[read, 0], joint_states[read, 1], np.asarray(ee, float), np.asarray(tail[0], float),
                      np.asarray(tail[1], float)]).astype(float)


def step_calls(involved, fixed, action, max_force: float) -> np.ndarray:
    """The simulator calls of one step(), in order, as call-log rows (:464-479): velocity control with force max_force on the
    involved joints, action[k] to involved[k]; then position control to 0 on the fixed joints, no force given; then one tick.
    Only then are reward, state and done read (:481-483)."""
    nan = float("nan")
    rows = [[CALL_MOTOR, j, VELOCITY_CONTROL, BY_VELOCITY, float(v), float(max_force)] for j, v in zip(involved, action)]
    rows += [[CALL_MOTOR, j, POSITION_CONTROL, BY_POSITION, 0.0, nan] for j in fixed]
    rows.append([CALL_TICK, -1, -1, -1, nan, nan])
    return np.array(rows, float)


def reset_calls(num_joints: int, initial_joint_positions, variation_range, uniform) -> np.ndarray:
    """The simulator calls of one reset(), in order (:281-301): the base to the origin; position control, no force given, on joint
    k = 0, 1, .. to 0 (neither list set), to initial[k] (only that set), to uniform(-var[k], var[k]) (only that set) or to
    uniform(initial[k] - var[k], initial[k] + var[k]) — one joint per pair of the two lists; then 50 ticks. `uniform` is Python's
    random.uniform (the global generator in the reference). A list that is None or empty counts as not set (:284)."""
    nan = float("nan")
    init = None if initial_joint_positions is None or len(initial_joint_positions) == 0 else list(initial_joint_positions)
    var = None if variation_range is None or len(variation_range) == 0 else list(variation_range)
    if init is None and var is None:
        goal = [0.0] * num_joints
    elif init is not None and var is not None:
        goal = [uniform(p - v, p + v) for p, v in zip(init, var)]
    elif init is not None:
        goal = init
    else:
        goal = [uniform(0 - v, 0 + v) for v in var]
    rows = [[CALL_BASE, -1, -1, -1, nan, nan]]
    rows += [[CALL_MOTOR, k, POSITION_CONTROL, BY_POSITION, float(p), nan] for k, p in enumerate(goal)]
    rows += [[CALL_TICK, -1, -1, -1, nan, nan]] * RESET_TICKS
    return np.array(rows, float)


BASE_POSE = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)      # position and quaternion of resetBasePositionAndOrientation (:281-282)


def relabelled(d_new_goal, contact: bool):
    """Hindsight: (reward, done) of a stored transition replayed towards another goal, d_new_goal away from where its step ended —
    the rule in free space, since a goal is only taken from a row that touched nothing; None for a row that records a contact,
    which keeps its reward and done."""
    if contact:
        return None
    return rule(d_new_goal, [MAX_DISTANCE], [], False)
