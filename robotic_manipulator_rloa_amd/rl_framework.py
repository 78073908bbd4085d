"""ManipulatorFramework: the user-facing object of the reference (rl_framework.py:47-699) re-hosted on the
MI355X hot path. Same method names, argument meaning, validation rules and exceptions; no compute happens
here — everything numeric goes through NAFAgent -> libnaf_hip.so.

Differences, all opt-in or forced by the image:
  * initialize_environment() needs PyBullet (absent from this image): it raises InvalidManipulatorFile with an
    explanatory message if `pybullet` cannot be imported; initialize_synthetic_environment() builds the
    kinematic stand-in (environment/synthetic.py) so the rest of the API works everywhere.
  * the demos take `interactive=False` to skip the reference's input() prompts (rl_framework.py:525,535) and
    `environment='synthetic'` to run without PyBullet.
  * p_mode / action_mode / use_graph can be passed to initialize_naf_agent(); defaults = reference semantics.
  * many-env training and evaluation: initialize_naf_agent(..., n_envs=E), run_training(...,
    n_envs=E) and test_trained_model(..., n_envs=E) run E copies of the configured environment — on the device for the
    synthetic stand-in, in E worker processes for anything else (PyBullet) — and produce what the one-env calls
    produce: the {episode: (score, last_frame)} dict, checkpoints/{episode}/weights.p + scores.txt, model.p, the logged
    test summary. Without n_envs every call is the reference's one-env loop, signature and behaviour untouched.
  * initialize_kinematic_environment() takes initialize_environment()'s arguments and builds the user's URDF arm as a
    kinematic chain under the reference's environment rule (environment/urdf_chain.py, environment/kinematic.py): one env
    on the host, n_envs=E on the device (csrc/chain_env.hip). Not a Bullet port: no dynamics, no mesh collision.
"""
from __future__ import annotations

import functools
import json
import os
import re
from dataclasses import dataclass, fields
from typing import List, Optional, Union

import numpy as np

from .arm_planner import ArmPlanner, _positive_int
from .arm_trajectory import TrajectoryMethods
from .environment.kinematic import (SCENE_CONDITIONS, Demonstrations, KinematicEnvironment, build_kinematic, cell_box_gaps,
                                    choose_scene)
from .environment.synthetic import SyntheticEnvironment
from .environment.urdf_chain import SCENE_TRIES, TARGET_THRESHOLD, cell_geometry_name
from .naf_components.naf_algorithm import NAFAgent
from .presets import ROBOT_PRESETS, pybullet_arguments, synthetic_initial_joints
from .utils.exceptions import (ConfigurationIncomplete, EnvironmentNotInitialized, InvalidEnvironmentParameter, InvalidHyperParameter,
                               InvalidManipulatorFile, InvalidNAFAgentParameter, MissingWeightsFile, NAFAgentNotInitialized)
from .utils.logger import Logger, get_global_logger

logger = get_global_logger()
Logger.set_logger_setup()


@dataclass
class HyperParameters:
    """Defaults of the reference (rl_framework.py:33-44)."""
    buffer_size: int = 100000
    batch_size: int = 128
    gamma: float = 0.99
    tau: float = 0.001
    learning_rate: float = 0.001
    update_freq: int = 1
    num_updates: int = 1


# accepted spellings -> (field, validity predicate, error text) — the reference's table (rl_framework.py:179-230),
# including its copy-pasted message for num_update
_HYPERPARAMETER_RULES = (
    (r'^(buffer_size|buffersize|BUFFER_SIZE|BUFFERSIZE)$', 'buffer_size', _positive_int,
     'Buffer Size is not an int or has a value lower than 0'),
    (r'^(batch_size|batchsize|BATCH_SIZE|BATCHSIZE)$', 'batch_size', _positive_int,
     'Batch Size is not an int or has a value lower than 0'),
    (r'^(gamma|GAMMA)$', 'gamma', lambda v: isinstance(v, (int, float)) and 0 < v < 1,
     'Gamma is not a float or its value is out of range (0, 1)'),
    (r'^(tau|TAU)$', 'tau', lambda v: isinstance(v, (int, float)) and 0 <= v <= 1,
     'Tau is not a float or its value is out of range [0, 1]'),
    (r'^(learning_rate|learningrate|LEARNING_RATE|LEARNINGRATE)$', 'learning_rate',
     lambda v: isinstance(v, (int, float)) and v > 0, 'Learning Rate is not a float or has a value lower than 0'),
    (r'^(update_freq|updatefreq|UPDATE_FREQ|UPDATEFREQ)$', 'update_freq', _positive_int,
     'Update Frequency is not an int or has a value lower than 0'),
    (r'^(num_update|numupdate|NUMUPDATE|NUM_UPDATE)$', 'num_updates', _positive_int,
     'Buffer Size is not an int or has a value lower than 0'),
)

# presets of run_demo_training / run_demo_testing (rl_framework.py:547-555, :571-580, :642-649, :669-678) plus the two
# robots BASELINE configs[3] / [4] name: one table, shared with the device env (presets.py)
_DEMO_ENVS = {name: pybullet_arguments(name) for name in ROBOT_PRESETS}


def _build_environment(manipulator_file: str, config_kwargs: dict):
    """Picklable factory of one PyBullet Environment (a worker process of environment.vector_env.HostVectorEnv calls it;
    workers never open a GUI: DIRECT mode, as north_star's "N independent PyBullet DIRECT envs per GPU")."""
    from .environment.environment import Environment, EnvironmentConfiguration
    return Environment(manipulator_file=manipulator_file,
                       environment_config=EnvironmentConfiguration(**dict(config_kwargs, visualize=False)))


def _build_synthetic(n_joints, target, obstacle, init, variation):
    return SyntheticEnvironment(n_joints, target, obstacle, init, variation)


# initialize_kinematic_environment's check of the scene ranges: (start pose, scene) draws of the twin, from a fixed seed
SCENE_CHECK_CASES = 1024
SCENE_CHECK_SEED = 20241017

# environments whose E copies are stepped on the device (everything else: E worker processes)
_DEVICE_ENVS = (SyntheticEnvironment, KinematicEnvironment)


class ManipulatorFramework(TrajectoryMethods):

    def __init__(self) -> None:
        self.env = None
        self.naf_agent: Optional[NAFAgent] = None
        self._env_factory = None          # picklable zero-argument factory of a copy of self.env (many-env paths)
        self._n_envs: Optional[int] = None
        self._hyperparameters: Optional[HyperParameters] = None
        self._initialize_hyperparameters()
        logger.info('The Framework has been initialized with the default hyperparameters configuration')

    def _initialize_hyperparameters(self) -> None:
        self._hyperparameters = HyperParameters()

    # ---- logging / info ------------------------------------------------------------------------------------------
    @staticmethod
    def set_log_level(log_level: int) -> None:
        names = {10: 'DEBUG', 20: 'INFO', 30: 'WARNING', 40: 'ERROR', 50: 'CRITICAL'}
        if log_level in names:
            logger.setLevel(log_level)
            logger.info(f'Log Level has been set to {log_level} ({names[log_level]})')
        else:
            logger.error(f'The Log level provided is invalid, so the previous Log Level is maintained ({logger.level}))')
            logger.error('Valid values: 10 (DEBUG), 20 (INFO), 30 (WARNING), 40 (ERROR), 50 (CRITICAL)')

    @staticmethod
    def get_required_hyperparameters() -> None:
        if logger.level > 10:
            logger.error('get_required_hyperparameters() only shows information for DEBUG log level. '
                         'Try running this method after setting the log level to DEBUG by calling '
                         'set_log_level(10) class method')
            return
        logger.debug('Required Hyperparameters:')
        for f in fields(HyperParameters):
            logger.debug('{:<25} default {}'.format(f.name, f.default))

    @staticmethod
    def plot_training_rewards(episode: int, mean_range: int = 50) -> None:
        """Mean reward per block of `mean_range` episodes from checkpoints/{episode}/scores.txt (rl_framework.py:124-157)."""
        try:
            with open(f'checkpoints/{episode}/scores.txt', 'r') as f:
                scores = json.loads(f.read())
        except FileNotFoundError as err:
            logger.error(f'File "scores.txt" located in checkpoints/{episode}/ folder was not found')
            raise err
        rewards = [result[0] for result in scores.values()]
        means = [sum(rewards[i:i + mean_range]) / mean_range for i in range(0, len(rewards) - mean_range + 1, mean_range)]
        import matplotlib.pyplot as plt   # optional dependency, only needed for this plot
        plt.plot(range(len(means)), means)
        plt.show()

    # ---- hyper-parameters ---------------------------------------------------------------------------------------
    def set_hyperparameter(self, hyperparameter: str, value: Union[float, int]) -> None:
        for pattern, field, valid, error in _HYPERPARAMETER_RULES:
            if re.match(pattern, hyperparameter):
                if not valid(value):
                    raise InvalidHyperParameter(error)
                setattr(self._hyperparameters, field, value)
                logger.info(f'Hyperparameter {hyperparameter} has been set to {value}')
                return
        raise InvalidHyperParameter(
            'The hyperparameter name passed as parameter is not valid. Valid hyperparameters are: '
            '["buffer_size", "batch_size", "gamma", "tau", "learning_rate", "update_freq", "num_update"]')

    # ---- pretrained weights -------------------------------------------------------------------------------------
    def _require_env_and_agent(self) -> None:
        if not self.env:
            raise EnvironmentNotInitialized
        if not self.naf_agent:
            raise NAFAgentNotInitialized

    def load_pretrained_parameters_from_weights_file(self, parameters_file_path: str) -> None:
        self._require_env_and_agent()
        self.naf_agent.initialize_pretrained_agent_from_weights_file(parameters_file_path)

    def load_pretrained_parameters_from_episode(self, episode: int) -> None:
        self._require_env_and_agent()
        self.naf_agent.initialize_pretrained_agent_from_episode(episode)

    # ---- configuration dumps ------------------------------------------------------------------------------------
    def get_environment_configuration(self) -> None:
        if not self.env:
            logger.error("Environment is not initialized yet, can't show configuration")
            return
        logger.info('Environment Configuration:')
        for label, attr in (('Manipulator File', 'manipulator_file'), ('End Effector index', 'endeffector_index'),
                            ('List of fixed Joints', 'fixed_joints'), ('List of Joints involved in training', 'involved_joints'),
                            ('Position of the Target', 'target_pos'), ('Position of the Obstacle', 'obstacle_pos'),
                            ('Initial position of joints', 'initial_joint_positions'),
                            ('Initial variation range of joints', 'initial_positions_variation_range'),
                            ('Max Force to be applied on joints', 'max_force'), ('Visualize mode', 'visualize')):
            logger.info('* {:<38} {}'.format(label + ':', getattr(self.env, attr, 'n/a')))
        if isinstance(self.env, KinematicEnvironment) and self.env.scene_ranges_on:
            for label, attr in (('Centre of the Target box', 'target_centre'), ('Half-widths of the Target box', 'target_range'),
                                ('Centre of the Obstacle box', 'obstacle_centre'),
                                ('Half-widths of the Obstacle box', 'obstacle_range'), ('Scene margin', 'scene_margin')):
                logger.info('* {:<38} {}'.format(label + ':', getattr(self.env, attr)))
        logger.info(f'* Instance of the Environment:         {self.env}')

    def get_nafagent_configuration(self) -> None:
        if not self.naf_agent:
            logger.error("NAFAgent is not initialized yet, can't show configuration")
            return
        logger.info('NAFAgent Configuration:')
        for label, attr in (('Environment Instance', 'environment'), ('State Size', 'state_size'),
                            ('Action Size', 'action_size'), ('Size of layers of the Neural Network', 'layer_size'),
                            ('Batch Size', 'batch_size'), ('Buffer Size', 'buffer_size'), ('Learning Rate', 'learning_rate'),
                            ('Tau', 'tau'), ('Gamma', 'gamma'), ('Update Frequency', 'update_freq'),
                            ('Number of Updates', 'num_updates'), ('Checkpoint frequency', 'checkpoint_frequency'),
                            ('Device', 'device')):
            logger.info('* {:<40} {}'.format(label + ':', getattr(self.naf_agent, attr)))

    # ---- evaluation -----------------------------------------------------------------------------------------------
    def test_trained_model(self, n_episodes: int, frames: int, n_envs: Optional[int] = None) -> dict:
        """n_episodes test episodes of at most `frames` steps; success iff done with reward == 250
        (rl_framework.py:319-367). Also returns the summary it logs. n_envs=E (or the n_envs given to
        initialize_naf_agent): the episodes are spread over E copies of the environment and every vector step is one
        batched act() — same result rule, same log lines."""
        if not self.naf_agent or not self.env:
            raise ConfigurationIncomplete
        results, num_collisions = [], 0
        E = n_envs if n_envs is not None else self._n_envs
        if E is not None and E > 1:
            triples = self._many_env_results(n_episodes, frames, int(E))
            results = [(ok, frame) for ok, frame, _ in triples]
            num_collisions = sum(1 for ok, _, done in triples if done and not ok)
            for ep in range(len(results)):
                logger.info('Test Episode number {ep} completed\n'.format(ep=ep + 1))
            n_episodes = 0
        for ep in range(n_episodes):
            state = self.env.reset()
            for frame in range(frames):
                action = self.naf_agent.act(state)
                state, reward, done = self.env.step(action)
                if done:
                    results.append((reward == 250, frame))
                    num_collisions += int(reward != 250)
                    break
                if frame == frames - 1:
                    results.append((False, frame))
            logger.info('Test Episode number {ep} completed\n'.format(ep=ep + 1))
        logger.info('RESULTS OF THE TEST:')
        for i, (ok, frame) in enumerate(results):
            logger.info(f'Results of Iteration {i + 1}: COMPLETED: {ok}. FRAMES: {frame}')
        wins = [f for ok, f in results if ok]
        summary = {'successes': len(wins), 'episodes': len(results), 'collisions': num_collisions,
                   'mean_frames_to_success': float(np.mean(wins)) if wins else float('nan')}
        logger.info(f'Number of successful executions: {len(wins)}/{len(results)}  '
                    f'({100.0 * len(wins) / max(1, len(results))}%)')
        logger.info(f'Average number of frames required to complete an episode: {summary["mean_frames_to_success"]}')
        logger.info(f'Number of episodes terminated because of collisions: {num_collisions}')
        return summary

    def reach_targets(self, targets, obstacles=None, initial_joint_positions=None, frames: int = 400, noise_scale: float = 0.0,
                      n_envs: Optional[int] = None, trajectories: bool = True, goal_poses: bool = False, joint_paths: bool = False,
                      certify: bool = False, roadmap: int = 0, shortcut: int = 0, orientations=None, approach_directions=None, tool_axis=(0.0, 0.0, 1.0),
                      orientation_tolerance: float = 1e-3, orientation_weight: Optional[float] = None,
                      avoid_contact: bool = False, clearance_goal: Optional[float] = None, push_iterations: int = 16):
        """Roll the trained policy out to GIVEN targets (kinematic environment only; on the device, thousands at once): query i
        starts at initial_joint_positions[i], with target targets[i] and obstacle obstacles[i], and runs until it reaches the
        target, touches the obstacle, itself or the workcell, or has taken `frames` steps. A query whose start pose is already in contact or at
        the target is not refused: its first step ends it (see start_* below).
          targets                 : [N][3], or [3] for a single query
          obstacles               : [N][3], [3] for all queries, or None: the environment's nominal obstacle
          initial_joint_positions : [N][A], [A] for all queries, or None: the environment's initial positions, no variation; one
                                    value per involved joint, in the order of involved_joints
          noise_scale             : 0 (default): the deterministic plan; 1: the exploration noise every act() of training has
          n_envs                  : envs per chunk of queries on the device (None: all queries at once, at most 4096)
        Returns an engine.ReachResult of numpy arrays over the queries: outcome ('reached' | 'obstacle' | 'self' | 'workcell' |
        'frames'), frames, final_distance, min_clearance, min_self_clearance, min_cell_clearance, score, joint_positions
        [N][frames + 1][A] (None with trajectories=False; a finished query repeats its final pose) and start_distance /
        start_clearance / start_self_clearance / start_cell_clearance, the measures at the start pose (the workcell's are +inf
        without a workcell). The agent is only read: training can go on afterwards.
        goal_poses=True (needs trajectories): the result's `goal` is solve_goal_poses() of the same queries and start poses, and
        `path_ratio` [N] the policy's joint path length — max-norm per frame, summed over its frames — over goal.joint_distance,
        NaN where the query did not reach or has no free goal pose. Both are None otherwise, and nothing else changes.
        joint_paths=True (implies goal_poses): the result's `path` is plan_joint_paths() from the start poses to goal's poses, with
        its defaults (queries without a reachable goal pose: outcome 'goal', NaN numbers), and `planned_ratio` [N] the same joint
        path length over path.length — a path that can be driven at its samples, where the straight line may not be — NaN where
        the query did not reach or no free path was found. Both are None otherwise, and nothing else changes.
        certify=True (with joint_paths): the paths are plan_joint_paths(certify=True)'s, and `path.certified` says which of them
        hold between their samples too.
        roadmap=M (with joint_paths, not with certify): the paths are plan_joint_paths(roadmap=M)'s; a query whose path is a
        'roadmap' polyline has its planned_ratio over that polyline's length.
        shortcut=W (with roadmap): the paths are plan_joint_paths(roadmap=M, shortcut=W)'s, and planned_ratio divides by the
        shortened length.
        orientations / approach_directions / tool_axis / orientation_tolerance / orientation_weight (with goal_poses or
        joint_paths): the goal poses are solve_goal_poses()'s with that orientation goal, and the paths lead to them. The
        rollout's own outcome stays positional — policy, observation and reward know no orientation: 'reached' says that the end
        effector came within the target threshold, whichever way it pointed.
        avoid_contact / clearance_goal / push_iterations (with goal_poses or joint_paths): solve_goal_poses()'s."""
        self._require_env_and_agent()
        planner = self._kinematic_planner('reach_targets', 'given-scene reset')
        if getattr(self.naf_agent, 'world_size', 1) > 1:
            raise InvalidNAFAgentParameter('reach_targets() answers a query on one GPU: not with a data-parallel agent')
        if n_envs is not None and not _positive_int(n_envs):
            raise InvalidNAFAgentParameter('Number of environments received is not a positive integer')
        return planner.reach_targets(self.naf_agent, targets, obstacles, initial_joint_positions, frames, noise_scale, n_envs,
                                     trajectories, goal_poses, joint_paths, certify, roadmap, shortcut,
                                     dict(orientations=orientations, approach_directions=approach_directions, tool_axis=tool_axis,
                                          orientation_tolerance=orientation_tolerance, orientation_weight=orientation_weight),
                                     dict(avoid_contact=avoid_contact, clearance_goal=clearance_goal, push_iterations=push_iterations))

    @functools.cached_property
    def arm_planner(self) -> ArmPlanner:
        """what the arm-planning methods delegate to, with its cache of device tools; made on first use, kept for good"""
        return ArmPlanner(self)

    def _kinematic_planner(self, who: str, lacking: str) -> ArmPlanner:
        """the planner, for a method that needs the kinematic environment"""
        if not self.env:
            raise EnvironmentNotInitialized
        if not isinstance(self.env, KinematicEnvironment):
            raise ConfigurationIncomplete(f'{who}() needs the kinematic environment (initialize_kinematic_environment()): '
                                          f'PyBullet and the synthetic stand-in have no {lacking}')
        return self.arm_planner

    def plan_joint_paths(self, targets=None, obstacles=None, initial_joint_positions=None, goal_joint_positions=None,
                         candidates: int = 16, resolution: float = 0.02, clearance_margin: float = 0.0, seed: int = 0,
                         on_device: Optional[bool] = None, certify: bool = False, roadmap: int = 0, shortcut: int = 0,
                         orientations=None, approach_directions=None, tool_axis=(0.0, 0.0, 1.0),
                         orientation_tolerance: float = 1e-3, orientation_weight: Optional[float] = None,
                         avoid_contact: bool = False, clearance_goal: Optional[float] = None, push_iterations: int = 16):
        """Collision-checked joint paths from start poses to goal poses (kinematic environment only; needs no agent): per query
        `candidates` joint-space polylines start -> via -> goal — candidate 0 through the midpoint, the straight line, the others
        through vias drawn around it from `seed` (environment/kinematic.py: path_vias) — are SAMPLED at poses at most `resolution`
        apart in the joints' max-norm (a multiple of 64 poses per path, at most 2048; beyond that the step is coarser and a warning
        says so once), each sample tested against the obstacle, the arm itself and the workcell under the rule of reach_targets()
        with clearance_margin to spare, and the shortest candidate with no blocked sample is returned. A free verdict holds AT THE
        SAMPLES; sample_step says how far apart they are. Without `certify` there is no continuous-collision certificate.
          targets              : [N][3] or [3]: the goal poses are solve_goal_poses(targets, ...) with its defaults and `seed`;
                                 queries without a reachable pose get outcome 'goal' and NaN numbers
          goal_joint_positions : [N][A] or [A]: the goal poses themselves. Exactly one of the two is given.
          orientations, approach_directions, tool_axis, orientation_tolerance, orientation_weight : with targets, the orientation
                                 goal of solve_goal_poses(); refused with goal_joint_positions
          avoid_contact, clearance_goal, push_iterations : with targets, solve_goal_poses()'s: goal poses that lean on something
                                 are pushed out of contact first, so fewer queries end 'goal'; refused with an orientation goal
          obstacles, initial_joint_positions : as reach_targets() takes them
          candidates           : 1 .. 64
          on_device            : None: the device when there is one; False: the float64 host twin under the same rule (slow)
          certify              : True: a candidate counts only when every test at every sample keeps clearance_margin plus how
                                 far the tested capsule can travel over half a sample interval (environment/kinematic.py:
                                 certify_joint_path) — then NO pose of the polyline, between the samples included, is closer than
                                 clearance_margin to anything. The shortest certified candidate wins; queries without one, or with
                                 a shorter candidate that is free at its samples only, are run again at twice the samples, up to
                                 2048. 'straight' and 'via' then name certified paths, the new outcome 'sampled' a path free at its
                                 samples only, and the result's certified, certified_slack and refinements are filled. The
                                 certificate is about the capsule model and the polyline; a controller's tracking error is not in it.
                                 On the device the certifying launch needs a little more LDS than the sampled one (a second
                                 reduction row and the tables of half-steps): an arm with pairs whose capsules only just fit a
                                 workgroup is refused there (NAF_CHAIN_ERR_LDS) though the sampled check serves it;
                                 on_device=False answers such an arm.
          roadmap              : M in 1 .. 62 (0, the default: none): every query that ends 'blocked' gets a roadmap of its own — its
                                 start pose, its goal pose and M milestones, half drawn around the straight line's midpoint as the
                                 vias are, half uniformly inside the joint limits, from `seed` (environment/kinematic.py:
                                 roadmap_milestones) — whose (M + 2)(M + 1) / 2 straight edges are sampled and tested as the
                                 candidates are, `resolution` apart; the shortest polyline start .. goal over the free edges is
                                 returned with the new outcome 'roadmap': candidate -1 and via NaN, length / the minima /
                                 sample_step / samples those of its edges, and the result's nodes [N][K][A] (NaN-padded), n_nodes
                                 and roadmap_free_edges filled (None without roadmap). Every other query is what it is without
                                 the argument. SAMPLED and random: 'blocked' after a roadmap is no proof that no path exists.
                                 Not together with certify: nothing certifies a roadmap's edges between their samples. An arm
                                 with a prismatic joint that has no limits is refused.
          shortcut             : W in 4 .. 64 (0, the default: none; needs roadmap): one shortcut round behind the roadmaps. Every
                                 'roadmap' polyline is subdivided to W nodes — its corners, and points handed to its longest
                                 pieces (environment/polyline.py: shortcut_nodes) — all W (W - 1) / 2 straight edges between
                                 them are sampled and tested by the same launch, and the shortest path over the free ones
                                 replaces the polyline where it is strictly shorter: nodes, n_nodes, length, the minima,
                                 sample_step and samples are then the new edges'. The result's roadmap_length [N] holds the
                                 lengths before the round (NaN: no roadmap path) and shortcut_free_edges [N] the free edges of
                                 each round (-1: none ran); both None without shortcut. One round, SAMPLED as the roadmap is.
        Returns environment.kinematic.JointPaths, arrays over the queries: outcome ('straight' | 'via' | 'blocked' | 'start' |
        'goal': the start / goal pose itself is blocked), candidate, via, length, straight_length, min_clearance,
        min_self_clearance, min_cell_clearance, straight_first_blocked, sample_step, samples; waypoints(n) resamples the paths."""
        planner = self._kinematic_planner('plan_joint_paths', 'chain model to solve on')
        return planner.plan_joint_paths(targets, obstacles, initial_joint_positions, goal_joint_positions, candidates, resolution,
                                        clearance_margin, seed, on_device, certify, roadmap, shortcut,
                                        dict(orientations=orientations, approach_directions=approach_directions, tool_axis=tool_axis,
                                             orientation_tolerance=orientation_tolerance, orientation_weight=orientation_weight),
                                        dict(avoid_contact=avoid_contact, clearance_goal=clearance_goal, push_iterations=push_iterations))

    def demonstrate_joint_paths(self, paths, targets=None, obstacles=None, speed: float = 1.0, frames: int = 400,
                                keep_contact: bool = False, on_device: Optional[bool] = None, polylines: bool = False):
        """Planned joint paths as demonstrations (kinematic environment only; needs no agent): query n drives the arm along
        paths' chosen polyline start -> via -> goal under the environment's own step rule, open loop — leg k in
        n_k = max(1, ceil(L_k / (speed DT))) ticks at one constant action, |a| <= speed — and every tick becomes the replay row
        run_training's environment would have written: an episode it could have produced. The poses follow the step's float32
        recurrence, so the arm reaches via and goal within its accumulated rounding (about 1e-4 rad at 400 ticks).
          paths        : JointPaths of plan_joint_paths(); queries with candidate < 0 get outcome 'none' — without polylines a
                         'roadmap' query among them: the two-leg launch drives two legs, and its polyline may have more
          targets      : [N][3], or None: the end effector at each path's goal pose; obstacles: as reach_targets() takes them
          speed        : 0 < speed <= 1, the share of the unit action — the policy's mean action is a tanh
          frames       : the episode budget, 1 .. 1024: a longer path is cut there (outcome 'frames')
          keep_contact : demonstrations that touch the obstacle, the arm or the workcell are dropped whole (the path was checked
                         at its samples only) unless this is set
          on_device    : None: the device when there is one; False: the float64 host twin, `rows` a numpy array (slow)
          polylines    : True: every query is planned as a polyline of any number of legs (environment/polyline.py:
                         demonstration_plan_legs; on the device naf_chain_demo_rows_legs) — a one-via query as its three nodes
                         start, via, goal, a 'roadmap' query as its nodes[:n_nodes], each leg under the per-leg rule above; only a
                         query with neither stands still and is 'none'. planned_ticks is then the sum over all legs.
        Returns environment.kinematic.Demonstrations: outcome ('reached' | 'frames' | 'end' | 'obstacle' | 'self' | 'workcell' |
        'none'), frames, final_distance, the three minima, planned_ticks, kept, rows [rows_total][row floats], rows_total."""
        planner = self._kinematic_planner('demonstrate_joint_paths', 'chain model to drive')
        return planner.demonstrate_joint_paths(paths, targets, obstacles, speed, frames, keep_contact, on_device, polylines)

    def certify_joint_paths(self, paths, obstacles=None, clearance_margin: float = 0.0, resolution: float = 0.02,
                            on_device: Optional[bool] = None):
        """Certificates for the polylines of planned joint paths, BETWEEN their samples (kinematic environment only; needs no
        agent): every query of `paths` that has a path — 'straight', 'via' and 'sampled' ones as start -> via -> goal, 'roadmap'
        ones as their nodes[:n_nodes], shortened by shortcut or not — is sampled leg by leg at poses at most `resolution` apart
        (a multiple of 64 per leg, at most 2048), and every test at every sample has to keep clearance_margin plus how far the
        tested capsule can travel over half a sample interval of that leg (environment/edge_certificate.py: certify_joint_edge).
        Then NO pose of the polyline is closer than clearance_margin to the obstacle, the arm itself or the workcell. A query
        that is free at its samples but not certified is run again with twice the samples on all its legs, up to 2048.
          paths            : JointPaths of plan_joint_paths(), of any kind; it is not changed
          obstacles        : as reach_targets() takes them — the scenes the paths were planned in
          clearance_margin : the distance every pose keeps where certified; resolution: the first round's sample step
          on_device        : None: the device when there is one (one naf_chain_edge_certify launch per chunk and round); False:
                             the float64 host twin under the same rule (slow). An arm with pairs whose capsules only just fit a
                             workgroup's LDS is refused on the device (NAF_CHAIN_ERR_LDS); on_device=False answers it.
        Returns environment.edge_certificate.PathCertificates, arrays over the queries: outcome ('certified' | 'sampled': free at
        the last round's samples, not certified at 2048 | 'blocked': a sample is below the margin | 'none': no path), certified,
        slack, leg_slack [N][Kmax - 1], weakest_leg, the three minima, samples, sample_step, refinements. The certificate is about
        the capsule model and the polyline; a controller's tracking error is not in it."""
        from .arm_certify import certify_joint_paths
        planner = self._kinematic_planner('certify_joint_paths', 'chain model to certify on')
        return certify_joint_paths(planner, paths, obstacles, clearance_margin, resolution, on_device)

    def plan_linear_moves(self, joint_positions, displacements, obstacles=None, hold: str = 'orientation',
                          tool_axis=(0.0, 0.0, 1.0), waypoints: int = 32, updates: int = 4, tolerance: float = 1e-3,
                          orientation_tolerance: float = 1e-3, resolution: float = 0.02, clearance_margin: float = 0.0,
                          reverse: bool = False, on_device: Optional[bool] = None):
        """Straight-line end-effector moves (kinematic environment only; needs no agent): from each given pose the end effector
        travels along a displacement in the world, orientation held — the last centimetres onto a part, the first ones away from
        it. The line is cut into `waypoints` equal parts; each waypoint is solved from the previous one's pose by `updates`
        damped least-squares updates (the ones of solve_goal_poses; environment/line_moves.py states the rule), so the joints
        follow one IK branch; then the joint-space legs between the waypoints are SAMPLED for collisions as plan_joint_paths
        samples its legs.
          joint_positions : [N][A], or [A] for one query: the poses the lines begin at (solve_goal_poses().joint_positions),
                            inside the limits
          displacements   : [N][3], or [3] for all queries: how far the end effector is to travel, metres in the world; not zero
          obstacles       : as reach_targets() takes them
          hold            : 'orientation': the end effector keeps the orientation it has at the given pose | 'axis': tool_axis (a
                            direction in the end-effector frame) keeps pointing where it points, the roll about it free |
                            'position': the orientation is free
          waypoints       : 1 .. 63; updates: at least 1, waypoints x updates <= 4096
          tolerance, orientation_tolerance : a waypoint is tracked iff it is within both of its line point and the held orientation
          resolution, clearance_margin     : the legs' sample step and the margin, as plan_joint_paths takes them
          reverse         : the nodes run from the far end to the given pose — the move is the approach; first_lost and
                            first_blocked_leg keep counting from the given pose
          on_device       : None: the device when there is one (one naf_chain_line_track launch and one naf_chain_edge_check
                            launch per chunk); False: the float64 host twin under the same rule (slow)
        Returns environment.line_moves.LinearMoves, arrays over the queries: outcome ('tracked' | 'lost': a waypoint missed a
        tolerance — a joint limit, the reach, a singularity | 'blocked': a leg of the tracked part has a blocked sample | 'start':
        the given pose is), fraction (the collision-free tracked share of the line), first_lost, first_blocked_leg, position_error,
        angle_error, joint_step, line_deviation (how far a leg's middle is from the line), the three minima, sample_step, samples,
        nodes [N][waypoints + 1][A], n_nodes, start, goal, end_effector_start, displacement. as_joint_paths() hands the 'tracked'
        lines to certify_joint_paths() and demonstrate_joint_paths(polylines=True)."""
        from .arm_line import plan_linear_moves
        planner = self._kinematic_planner('plan_linear_moves', 'chain model to track a line on')
        return plan_linear_moves(planner, joint_positions, displacements, obstacles, hold, tool_axis, waypoints, updates, tolerance,
                                 orientation_tolerance, resolution, clearance_margin, reverse, on_device)

    def _check_demonstrations(self, demos, E) -> None:
        if not isinstance(demos, Demonstrations):
            raise InvalidNAFAgentParameter('demonstrations is the Demonstrations that demonstrate_joint_paths() returned')
        if not isinstance(self.env, KinematicEnvironment):
            raise ValueError('demonstrations need the kinematic arm environment (a chain model on the device): the synthetic '
                             'stand-in and PyBullet have no planned joint paths')
        if E is None or E <= 1:
            raise ValueError('demonstrations need n_envs > 1: the one-env loop does not read device rows')

    def add_demonstrations(self, demos) -> dict:
        """Append the kept rows of `demos` (demonstrate_joint_paths()) to the agent's replay ring, in query order then tick order.
        Returns the counts run_training(demonstrations=) leaves in last_run_stats."""
        if not self.naf_agent or not self.env:
            raise ConfigurationIncomplete
        self._check_demonstrations(demos, 2)
        return self.naf_agent.add_demonstrations(demos)

    def solve_goal_poses(self, targets, obstacles=None, initial_joint_positions=None, restarts: int = 8, iterations: int = 32,
                         tolerance: float = 1e-3, clearance_margin: float = 0.0, seed: int = 0, on_device: Optional[bool] = None,
                         orientations=None, approach_directions=None, tool_axis=(0.0, 0.0, 1.0),
                         orientation_tolerance: float = 1e-3, orientation_weight: Optional[float] = None,
                         avoid_contact: bool = False, clearance_goal: Optional[float] = None, push_iterations: int = 16):
        """Joint values that put the end effector on GIVEN targets (kinematic environment only; needs no agent): per query a
        damped least-squares iteration on the end effector's positional Jacobian from `restarts` seeds — the start pose and
        restarts - 1 poses drawn uniformly inside the limits from `seed` — for `iterations` updates each, then the choice among
        them: a converged (|target - end effector| <= tolerance) pose that keeps clearance_margin from the obstacle, the arm itself
        and the workcell before a converged one in contact before the nearest miss, and among equals the one nearest the start
        pose in the joints' max-norm (environment/kinematic.py: ik_step, select_goal_pose). Contact plays no part in the iteration.
          targets, obstacles, initial_joint_positions : as reach_targets() takes them
          restarts    : a power of two, 1 .. 64
          on_device   : None: the device when there is one; False: the float64 host twin under the same rule (slow: a chain walk
                        per update and candidate)
          orientations        : [N][4], or [4] for all queries: the end effector's orientation in the world as a quaternion
                                (x, y, z, w), the convention of a URDF / PyBullet link orientation (it is scaled to unit length)
          approach_directions : [N][3], or [3] for all queries: a direction in the world that tool_axis, a direction in the
                                end-effector frame (default its z axis), is to point along — [0, 0, -1] approaches from above; the
                                roll about it is free. At most one of the two is given; neither: position only, as before.
          orientation_tolerance : radians; with an orientation goal a pose is converged iff |target - end effector| <= tolerance
                                and the angle left to the goal <= orientation_tolerance
          orientation_weight  : metres per radian, how a radian of angular error weighs against a metre (None: 0.25 reach)
          avoid_contact       : True: between the iteration and the choice every converged candidate that is closer than
                                clearance_goal to the obstacle, the arm itself or the workcell is refined on the device (or by the
                                twin) by push_iterations updates that hold the end effector on the target and push the pose away
                                from its least clearance in the task's null space (environment/kinematic.py: refine_goal_poses);
                                a candidate is never worse than it came in. Positional goals only: refused together with
                                orientations or approach_directions. The result's pushed [N] and input_clearance [N] are then
                                filled (None otherwise).
          clearance_goal      : the clearance the push aims for (None: clearance_margin + 0.02)
        With an orientation goal the iteration runs on the 6-row Jacobian of position and orientation (environment/kinematic.py:
        orientation_error, ik_pose_step), and the result's angle_residual [N] holds the angle left at the chosen pose.
        Returns environment.kinematic.GoalPoses, arrays over the queries: reachable, free, joint_positions [N][A], residual,
        clearance, self_clearance, cell_clearance, joint_distance, restart, converged_restarts; angle_residual is None without an
        orientation goal."""
        planner = self._kinematic_planner('solve_goal_poses', 'chain model to solve on')
        return planner.solve_goal_poses(targets, obstacles, initial_joint_positions, restarts, iterations, tolerance, clearance_margin,
                                        seed, on_device,
                                        dict(orientations=orientations, approach_directions=approach_directions, tool_axis=tool_axis,
                                             orientation_tolerance=orientation_tolerance, orientation_weight=orientation_weight),
                                        dict(avoid_contact=avoid_contact, clearance_goal=clearance_goal, push_iterations=push_iterations))

    # ---- environment ------------------------------------------------------------------------------------------------
    def initialize_environment(self, manipulator_file: str, endeffector_index: int, fixed_joints: List[int],
                               involved_joints: List[int], target_position: List[float], obstacle_position: List[float],
                               initial_joint_positions: List[float] = None,
                               initial_positions_variation_range: List[float] = None, max_force: float = 200.,
                               visualize: bool = True) -> None:
        """PyBullet environment (rl_framework.py:369-417). The simulator is third-party and not part of this build."""
        try:
            from .environment.environment import Environment, EnvironmentConfiguration
        except ImportError as e:
            raise InvalidManipulatorFile(
                f'PyBullet is not importable here ({e}); use initialize_synthetic_environment() for the built-in '
                f'kinematic stand-in, or install pybullet to load {manipulator_file}') from e
        config = EnvironmentConfiguration(
            endeffector_index=endeffector_index, fixed_joints=fixed_joints, involved_joints=involved_joints,
            target_position=target_position, obstacle_position=obstacle_position,
            initial_joint_positions=initial_joint_positions,
            initial_positions_variation_range=initial_positions_variation_range, max_force=max_force, visualize=visualize)
        self.env = Environment(manipulator_file=manipulator_file, environment_config=config)
        self._env_factory = functools.partial(_build_environment, manipulator_file, dict(
            endeffector_index=endeffector_index, fixed_joints=fixed_joints, involved_joints=involved_joints,
            target_position=target_position, obstacle_position=obstacle_position,
            initial_joint_positions=initial_joint_positions,
            initial_positions_variation_range=initial_positions_variation_range, max_force=max_force))
        logger.info('Pybullet Environment successfully initialized')

    def initialize_synthetic_environment(self, n_joints: int = 6, target_position: List[float] = None,
                                         obstacle_position: List[float] = None, initial_joint_positions: List[float] = None,
                                         initial_positions_variation_range: List[float] = None,
                                         obstacle_jitter: float = 0.0) -> None:
        """obstacle_jitter (many-env runs on the device only): each env's obstacle sits at obstacle_position + U(-j, j)^3,
        drawn once per (rank, env) — BASELINE configs[3]'s "randomized obstacle_position per env"."""
        self.env = SyntheticEnvironment(n_joints, target_position, obstacle_position, initial_joint_positions,
                                        initial_positions_variation_range)
        self._obstacle_jitter = float(obstacle_jitter)
        self._env_factory = functools.partial(_build_synthetic, n_joints, target_position, obstacle_position,
                                              initial_joint_positions, initial_positions_variation_range)
        logger.info('Synthetic (kinematic stand-in) Environment successfully initialized')

    def initialize_kinematic_environment(self, manipulator_file: str, endeffector_index: int, fixed_joints: List[int],
                                         involved_joints: List[int], target_position: List[float],
                                         obstacle_position: List[float], initial_joint_positions: List[float] = None,
                                         initial_positions_variation_range: List[float] = None, link_radius: float = 0.0,
                                         obstacle_radius: float = 0.06, obstacle_jitter: float = 0.0, max_force: float = 200.,
                                         visualize: bool = False, consider_autocollision: bool = False,
                                         autocollision_ignore: Optional[list] = None, target_range: Optional[List[float]] = None,
                                         obstacle_range: Optional[List[float]] = None, scene_margin: float = 0.02,
                                         floor_height: Optional[float] = None, workcell_planes: Optional[list] = None,
                                         workcell_spheres: Optional[list] = None, cell_ignore: Optional[list] = None,
                                         workcell_boxes: Optional[list] = None) -> None:
        """initialize_environment()'s arguments (rl_framework.py:369-417) for the built-in kinematic environment: the arm of
        `manipulator_file` (a URDF) as a serial chain under the reference's environment rule, velocity control applied exactly.
        Not a Bullet port — no dynamics (max_force is accepted and ignored), no mesh collision (links are capsules of their
        primitive collision radius, else link_radius), no GUI (visualize=True is refused). obstacle_jitter: as
        initialize_synthetic_environment's. One env runs on the host, n_envs=E copies run on the device.
        consider_autocollision: initialize_environment()'s switch — contact between the capsules of two links that are not
        neighbours ends the episode with -1000 (environment.py:311-371, :394-412); pairs that the capsules keep in contact at
        every pose are dropped when the model is compiled (env.model.self_pairs_dropped), autocollision_ignore (pairs of link
        names or link indices) drops more. A start pose in self-contact is refused here.
        target_range / obstacle_range: half-widths [x, y, z] of the boxes around target_position / obstacle_position. Every
        episode, of the host env and of each device env, then gets a target and an obstacle of its own from them: up to 8
        candidates are drawn and the first one is taken whose target is farther than 0.05 + scene_margin from the start pose's
        end effector, whose obstacle is scene_margin clear of the arm at the start pose and whose target is not inside the
        obstacle; if none is, the episode runs in the nominal scene. Ranges that put the scene on the arm — more than half of
        1024 sampled episode starts falling back — are refused here. Not together with obstacle_jitter.
        floor_height / workcell_planes / workcell_spheres: the fixed geometry of the cell the arm stands in — a floor z >= z0,
        half-spaces (nx, ny, nz, d) with a unit normal and the free side n.x - d >= 0, spheres (cx, cy, cz, r), 16 in all. A
        capsule that touches one ends the episode with -1000, as obstacle contact does; the geometry is the same in every
        episode and is not part of the state. (Capsule, geometry) pairs in contact at every pose — the base on the floor — are
        dropped when the model is compiled (env.model.cell_pairs_dropped), cell_ignore [(link, geometry index)] drops more;
        geometry indices count the spheres first, then the floor, then workcell_planes. Refused here: a start pose in
        workcell contact, a target (or, with target_range, a point of its box) within 0.05 (+ scene_margin) of a geometry,
        and initial_positions_variation_range under which more than half of 1024 sampled episode starts are in workcell
        contact. PyBullet and the stand-in environment have no workcell.
        workcell_boxes: rounded oriented boxes among those 16 — the table top with its edge, a shelf, a post — each
        [cx, cy, cz, hx, hy, hz] (centre and half extents), [.., roll, pitch, yaw] (the URDF convention of a joint origin's rpy)
        or [.., roll, pitch, yaw, r] with a rounding radius r: zero half extents and r > 0 give a fixed capsule or a rounded
        plate. Clearance of a capsule: distance(its axis, box) - its radius - r; an axis that enters the box is at distance 0,
        so min_cell_clearance of reach_targets reads -(radius + r) there: no penetration depth is reported. Geometry indices
        count the boxes last. The same refusals hold for boxes."""
        if visualize:
            raise InvalidManipulatorFile('the kinematic environment has no visualisation: pass visualize=False '
                                         '(initialize_environment() opens the PyBullet GUI)')
        for label, r in (('Target range', target_range), ('Obstacle range', obstacle_range)):
            if r is None:
                continue
            if not isinstance(r, list) or len(r) != 3:
                raise InvalidEnvironmentParameter(f'{label} received is not a list of three half-widths')
            if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v) and v >= 0 for v in r):
                raise InvalidEnvironmentParameter(f'An item inside the {label} list is not a non-negative number')
        if isinstance(scene_margin, bool) or not isinstance(scene_margin, (int, float)) or not scene_margin >= 0:
            raise InvalidEnvironmentParameter('Scene margin received is not a non-negative number')
        ranged = any(v > 0 for r in (target_range, obstacle_range) if r is not None for v in r)
        if ranged and obstacle_jitter > 0:
            raise ValueError('obstacle_jitter moves each env\'s obstacle once, target_range / obstacle_range draw a scene every '
                             'episode: give one or the other')
        args = (manipulator_file, endeffector_index, list(fixed_joints), list(involved_joints), list(target_position),
                list(obstacle_position), None if initial_joint_positions is None else list(initial_joint_positions),
                None if initial_positions_variation_range is None else list(initial_positions_variation_range),
                float(link_radius), float(obstacle_radius), bool(consider_autocollision),
                None if autocollision_ignore is None else [tuple(p) for p in autocollision_ignore])
        if floor_height is not None and (isinstance(floor_height, bool) or not isinstance(floor_height, (int, float))
                                         or not np.isfinite(floor_height)):
            raise InvalidEnvironmentParameter('Floor height received is not a finite number')
        for label, geoms in (('Workcell planes', workcell_planes), ('Workcell spheres', workcell_spheres)):
            if geoms is None:
                continue
            if not isinstance(geoms, (list, tuple)) or not all(isinstance(g, (list, tuple)) and len(g) == 4 for g in geoms):
                raise InvalidEnvironmentParameter(f'{label} received is not a list of four-number entries')
            if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v) for g in geoms for v in g):
                raise InvalidEnvironmentParameter(f'An item inside the {label} list is not a finite number')
        if workcell_boxes is not None:
            if not isinstance(workcell_boxes, (list, tuple)) or not all(isinstance(g, (list, tuple)) and len(g) in (6, 9, 10)
                                                                        for g in workcell_boxes):
                raise InvalidEnvironmentParameter('Workcell boxes received is not a list of entries of 6, 9 or 10 numbers')
            if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v) for g in workcell_boxes for v in g):
                raise InvalidEnvironmentParameter('An item inside the Workcell boxes list is not a finite number')
        scene_kw = dict(target_range=None if target_range is None else [float(v) for v in target_range],
                        obstacle_range=None if obstacle_range is None else [float(v) for v in obstacle_range],
                        scene_margin=float(scene_margin), floor_height=None if floor_height is None else float(floor_height),
                        workcell_planes=None if workcell_planes is None else [tuple(float(v) for v in g) for g in workcell_planes],
                        workcell_spheres=None if workcell_spheres is None else [tuple(float(v) for v in g) for g in workcell_spheres],
                        cell_ignore=None if cell_ignore is None else [tuple(p) for p in cell_ignore])
        if workcell_boxes:      # (a box-free call keeps the factory's arguments it always had)
            scene_kw['workcell_boxes'] = [tuple(float(v) for v in g) for g in workcell_boxes]
        env = build_kinematic(*args, **scene_kw)
        if env.model.cell_pairs:
            self._check_workcell(env, manipulator_file)
        if ranged:
            self._check_scene_ranges(env, manipulator_file)
        if env.model.self_pairs:
            clear = env.pair_clearances(env.initial_joint_positions)
            worst = int(np.argmin(clear))
            if clear[worst] < 0.0:
                a, b = (env.model.segments[s].link_name for s in env.model.self_pairs[worst])
                raise ValueError(f'{manipulator_file}: at the initial joint positions the links {a!r} and {b!r} are in '
                                 f'self-contact (clearance {clear[worst]:.4f} m between their capsules): every episode would end at '
                                 f'its first step. Choose another start pose or a smaller link_radius, or pass '
                                 f'autocollision_ignore=[({a!r}, {b!r})]')
        self.env = env
        self._obstacle_jitter = float(obstacle_jitter)
        self._env_factory = functools.partial(build_kinematic, *args, **scene_kw)
        logger.info(f'Kinematic Environment successfully initialized from {manipulator_file} '
                    f'({self.env.model.A} driven joints, {len(self.env.model.segments)} collision capsules)')

    @staticmethod
    def _check_workcell(env: KinematicEnvironment, manipulator_file: str) -> None:
        """Refuses a nominal start pose in workcell contact, a target (box) too near a geometry and start ranges under which more
        than half of SCENE_CHECK_CASES sampled episode starts are in workcell contact; logs that share otherwise."""
        model = env.model
        pairs = model.cell_pairs
        clear = env.cell_clearances(env.initial_joint_positions)
        worst = int(np.argmin(clear))
        if clear[worst] < 0.0:
            s, g = pairs[worst]
            raise ValueError(f'{manipulator_file}: at the initial joint positions the link {model.segments[s].link_name!r} is in '
                             f'contact with {cell_geometry_name(model, g)} (clearance {clear[worst]:.4f} m): every episode would '
                             f'end at its first step. Choose another start pose, move the geometry, or pass '
                             f'cell_ignore=[({model.segments[s].link_name!r}, {g})]')
        need = TARGET_THRESHOLD + (env.scene_margin if env.scene_ranges_on else 0.0)
        gaps = cell_box_gaps(model, env.target_centre, env.target_range)
        g = int(np.argmin(gaps))
        if gaps[g] < need:
            what = (f'the target box (target_position +- target_range) comes within {gaps[g]:.4f} m' if env.scene_ranges_on
                    else f'the target lies within {gaps[g]:.4f} m')
            raise ValueError(f'{manipulator_file}: {what} of {cell_geometry_name(model, g)}; a target needs {need:.4f} m (the 0.05 of '
                             f'the reward rule' + (' + scene_margin' if env.scene_ranges_on else '') + ') so that the arm can '
                             f'reach it without touching the workcell')
        rng = np.random.default_rng(SCENE_CHECK_SEED)
        init, var = np.array([j.init for j in model.joints]), np.array([j.variation for j in model.joints])
        touching = int(np.sum(env.cell_clearance(init + rng.uniform(-1.0, 1.0, (SCENE_CHECK_CASES, len(init))) * var) < 0.0))
        if touching > SCENE_CHECK_CASES // 2:
            raise ValueError(f'{manipulator_file}: {touching} of {SCENE_CHECK_CASES} sampled episode starts (initial joint positions '
                             f'+- initial_positions_variation_range) are in workcell contact and would end at their first step: '
                             f'narrow the variation range, choose another start pose or move the geometry')
        boxes = f', {len(model.cell_boxes)} boxes' if model.cell_boxes else ''
        logger.info(f'Workcell: {len(model.cell_spheres)} spheres, {len(model.cell_planes)} half-spaces{boxes}, {len(pairs)} tested pairs; '
                    f'{100.0 * touching / SCENE_CHECK_CASES:.1f}% of {SCENE_CHECK_CASES} sampled episode starts are in workcell '
                    f'contact')

    @staticmethod
    def _check_scene_ranges(env: KinematicEnvironment, manipulator_file: str) -> None:
        """SCENE_CHECK_CASES (start pose, scene) draws of the twin from a fixed seed: logs how many take a candidate, and refuses
        ranges under which more than half fall back to the nominal scene."""
        rng = np.random.default_rng(SCENE_CHECK_SEED)
        joints = env.model.joints
        init, var = np.array([j.init for j in joints]), np.array([j.variation for j in joints])
        q0 = init + rng.uniform(-1.0, 1.0, (SCENE_CHECK_CASES, len(joints))) * var
        _, _, index, margins = choose_scene(env, q0, rng.random((SCENE_CHECK_CASES, SCENE_TRIES, 6)))
        fallback, first = int(np.sum(index < 0)), int(np.sum(index == 0))
        tried = np.arange(SCENE_TRIES) < np.where(index < 0, SCENE_TRIES, index)[:, None]      # the candidates before the choice
        rejects = np.sum((margins < 0.0) & tried[..., None], axis=(0, 1))
        rate = 1.0 - fallback / SCENE_CHECK_CASES
        logger.info(f'Scene ranges: {100.0 * rate:.1f}% of {SCENE_CHECK_CASES} sampled episode starts take a drawn scene '
                    f'({100.0 * first / SCENE_CHECK_CASES:.1f}% the first candidate), {100.0 * (1.0 - rate):.1f}% fall back to the '
                    f'nominal scene')
        if fallback > SCENE_CHECK_CASES // 2:
            raise ValueError(f'{manipulator_file}: with these target_range / obstacle_range {fallback} of {SCENE_CHECK_CASES} sampled '
                             f'episode starts find no admissible scene among {SCENE_TRIES} candidates and fall back to the nominal '
                             f'one; most rejections: {SCENE_CONDITIONS[int(np.argmax(rejects))]} (condition '
                             f'{int(np.argmax(rejects)) + 1}, {int(rejects.max())} candidates). The ranges put the scene on the arm: '
                             f'move the boxes away from it or make them larger')

    def delete_environment(self) -> None:
        if not self.env:
            logger.error('No existing instance of Environment found')
            return
        close = getattr(self.env, 'close', None)
        if close:
            close()
        self.env = None
        self._env_factory = None
        logger.info('Environment instance has been successfully removed')

    # ---- agent --------------------------------------------------------------------------------------------------------
    def initialize_naf_agent(self, checkpoint_frequency: int = 500, seed: int = 0, n_envs: Optional[int] = None,
                             **agent_options) -> None:
        """rl_framework.py:431-465: same guards, same NAFAgent keyword arguments (layer_size is 256, :452).
        The device is cuda:0 — this build has no CPU path, so a missing GPU is an error, not a silent fallback.
        n_envs=E: run_training / test_trained_model of this agent use E copies of the environment (see the module text)."""
        if not self.env:
            raise EnvironmentNotInitialized
        if not isinstance(checkpoint_frequency, int) or not isinstance(seed, int):
            raise InvalidNAFAgentParameter('Checkpoint Frequency or Seed received is not an integer')
        if n_envs is not None and (not isinstance(n_envs, int) or n_envs < 1):
            raise InvalidNAFAgentParameter('Number of environments received is not a positive integer')
        self._n_envs = n_envs
        hp = self._hyperparameters
        from .parallel import local_device
        device = local_device()              # cuda:LOCAL_RANK — one process per GPU under torch.distributed.run
        self.naf_agent = NAFAgent(environment=self.env,
                                  state_size=self.env.observation_space.shape[0],
                                  action_size=self.env.action_space.shape[0],
                                  layer_size=256,
                                  batch_size=hp.batch_size, buffer_size=hp.buffer_size, learning_rate=hp.learning_rate,
                                  tau=hp.tau, gamma=hp.gamma, update_freq=hp.update_freq, num_updates=hp.num_updates,
                                  checkpoint_frequency=checkpoint_frequency, device=device, seed=seed, **agent_options)
        logger.info('NAF Agent successfully initialized')

    def delete_naf_agent(self) -> None:
        if not self.naf_agent:
            logger.error('No existing instance of NAFAgent found')
            return
        self.naf_agent = None
        self._n_envs = None
        logger.info('NAFAgent instance has been successfully removed')

    # ---- training ---------------------------------------------------------------------------------------------------
    def run_training(self, episodes: int, frames: Optional[int] = 500, verbose: bool = True, n_envs: Optional[int] = None,
                     hindsight: float = 0.0, hindsight_horizon: Optional[int] = None, demonstrations=None):
        """rl_framework.py:478-501 -> NAFAgent.run(frames, episodes, verbose): {episode: (score, last_frame)}, checkpoints,
        model.p. n_envs=E (or the n_envs given to initialize_naf_agent): the same outputs from E environments at once —
        episodes numbered in completion order, `frames` the budget of each; counters in naf_agent.last_run_stats.
        hindsight / hindsight_horizon (kinematic environment with n_envs=E only): NAFAgent.run_vectorized's hindsight goals.
        demonstrations (kinematic environment with n_envs=E only): the Demonstrations of demonstrate_joint_paths(), whose kept rows
        seed the replay ring before the first tick; not together with hindsight, not on a resume."""
        if not self.naf_agent or not self.env:
            raise ConfigurationIncomplete
        E = n_envs if n_envs is not None else self._n_envs
        hs = self._hindsight_arguments(hindsight, hindsight_horizon, E)
        if demonstrations is not None:
            self._check_demonstrations(demonstrations, E)
            hs = dict(hs, demonstrations=demonstrations)
        if E is None or E <= 1:
            return self.naf_agent.run(frames, episodes, verbose)
        if isinstance(self.env, _DEVICE_ENVS):
            return self.naf_agent.run_vectorized(episodes=episodes, n_envs=int(E), max_frames=frames, verbose=verbose, **hs,
                                                 **self._device_env_arguments())['scores']
        vec = self._host_vector_env(int(E), frames)
        try:
            return self.naf_agent.run_host_vectorized(vec, episodes=episodes, verbose=verbose)['scores']
        finally:
            vec.close()

    def _hindsight_arguments(self, hindsight, hindsight_horizon, E) -> dict:
        """run_vectorized's two arguments, or nothing for a call without them; a refusal where no kinematic many-env loop runs"""
        if not hindsight and hindsight_horizon is None:
            return {}
        from .utils.hindsight import check_arguments
        check_arguments(hindsight, 1 if hindsight_horizon is None else hindsight_horizon)
        if hindsight and (E is None or E <= 1 or not isinstance(self.env, KinematicEnvironment)):
            raise ValueError('hindsight goals need the kinematic arm environment with n_envs > 1 (a chain model on the device): '
                             'the one-env loop, the synthetic stand-in and PyBullet store no goal the gather could rewrite')
        return {'hindsight': float(hindsight), 'hindsight_horizon': hindsight_horizon}

    def resume_training(self, episode: int, episodes: int, frames: Optional[int] = 500, verbose: bool = True,
                        n_envs: Optional[int] = None, hindsight: float = 0.0, hindsight_horizon: Optional[int] = None,
                        demonstrations=None):
        """Continue the run_training() whose checkpoint `episode` holds a training_state.pt (an agent initialised with
        save_training_state=True writes one beside weights.p) up to `episodes` episodes: the same run as if it had never
        stopped. Returns the whole scores dict. frames / n_envs must be those of the saved run."""
        if not self.naf_agent or not self.env:
            raise ConfigurationIncomplete
        if demonstrations is not None:
            raise ValueError('demonstrations cannot be added on a resume: the saved ring, demonstrations included, is already in '
                             'the training state')
        if not isinstance(episode, int) or isinstance(episode, bool) or episode < 1:
            raise InvalidNAFAgentParameter('The checkpoint episode received is not a positive integer')
        if not isinstance(episodes, int) or isinstance(episodes, bool) or episodes < episode:
            raise InvalidNAFAgentParameter('The episode budget received is not an integer at least as large as the checkpoint')
        E = n_envs if n_envs is not None else self._n_envs
        if E is not None and E > 1 and not isinstance(self.env, _DEVICE_ENVS):
            raise InvalidNAFAgentParameter('Training with environments in worker processes cannot be resumed')
        hs = self._hindsight_arguments(hindsight, hindsight_horizon, E)
        path = f'checkpoints/{episode}/training_state.pt'
        if not os.path.isfile(path):
            raise MissingWeightsFile(f'{path} does not exist (initialize the agent with save_training_state=True)')
        self.naf_agent.load_training_state(path)
        if E is None or E <= 1:
            return self.naf_agent.run(frames, episodes, verbose, resume=True)
        return self.naf_agent.run_vectorized(episodes=episodes, n_envs=int(E), max_frames=frames, verbose=verbose, resume=True,
                                             **hs, **self._device_env_arguments())['scores']

    def run_vectorized_training(self, vector_steps: int, n_envs: int = 64, max_frames: int = 400) -> dict:
        """Many-env training on the device-resident synthetic arms (BASELINE configs[1..4] shape) for a fixed number of
        vector steps; see NAFAgent.run_vectorized (counters + 'scores')."""
        if not self.naf_agent or not self.env:
            raise ConfigurationIncomplete
        kw = self._device_env_arguments() if isinstance(self.env, _DEVICE_ENVS) else {}
        return self.naf_agent.run_vectorized(vector_steps, n_envs=n_envs, max_frames=max_frames, **kw)

    # ---- E copies of the configured environment -------------------------------------------------------------------
    def _device_env_arguments(self) -> dict:
        """The synthetic environment's configuration as csrc/synth_env.hip takes it; the kinematic environment's chain model
        and scene (csrc/chain_env.hip)."""
        env = self.env
        if isinstance(env, KinematicEnvironment):
            scene = {'target': [float(x) for x in env.target_pos], 'obstacle': [float(x) for x in env.obstacle_pos],
                     'obstacle_radius': env.obstacle_radius, 'obstacle_jitter': getattr(self, '_obstacle_jitter', 0.0)}
            if env.scene_ranges_on:      # target_pos / obstacle_pos are then some episode's scene: the device draws around the centres
                scene.update(target=[float(x) for x in env.target_centre], obstacle=[float(x) for x in env.obstacle_centre],
                             target_range=[float(x) for x in env.target_range],
                             obstacle_range=[float(x) for x in env.obstacle_range], scene_margin=env.scene_margin)
            return {'chain': env.model, 'scene': scene}
        pad8 = lambda v: ([float(x) for x in v] + [0.0] * 8)[:8]          # noqa: E731
        var = env.initial_positions_variation_range
        return {'preset': pad8(env.initial_joint_positions) + [float(x) for x in env.target_pos] +
                [float(x) for x in env.obstacle_pos], 'variation': pad8(var) if var is not None else [0.0] * 8,
                'obstacle_jitter': getattr(self, '_obstacle_jitter', 0.0)}

    def _host_vector_env(self, n_envs: int, frames: int):
        from .environment.vector_env import HostVectorEnv
        if self._env_factory is None:
            raise ConfigurationIncomplete('many-env runs need an environment built by initialize_environment() / '
                                          'initialize_synthetic_environment() (a factory of copies of it)')
        return HostVectorEnv(self._env_factory, n_envs, self.naf_agent.state_size, self.naf_agent.action_size,
                             max_frames=frames, seed=self.naf_agent.seed)

    def _many_env_results(self, n_episodes: int, frames: int, n_envs: int):
        if isinstance(self.env, _DEVICE_ENVS):
            return self.naf_agent.evaluate_vectorized(n_episodes, frames, n_envs=n_envs, **self._device_env_arguments())
        vec = self._host_vector_env(n_envs, frames)
        try:
            return self.naf_agent.evaluate_host_vectorized(vec, n_episodes)
        finally:
            vec.close()

    # ---- demos --------------------------------------------------------------------------------------------------------
    def _clear_for_demo(self, interactive: bool) -> bool:
        for what, present, delete in (('Environment', self.env, self.delete_environment),
                                      ('NAFAgent', self.naf_agent, self.delete_naf_agent)):
            if present:
                if interactive and input(f'{what} instance found. Overwrite? [Y/n] ').lower() != 'y':
                    logger.info(f'Demo could not run due to the presence of a user-configured {what} instance')
                    return False
                delete()
        return True

    def _demo_environment(self, robot: str, environment: str, variation, visualize: bool) -> None:
        preset = dict(_DEMO_ENVS[robot])
        if environment == 'synthetic':
            n = len(preset['involved_joints'])
            self.initialize_synthetic_environment(n, preset['target_position'], preset['obstacle_position'],
                                                  synthetic_initial_joints(robot), list(variation)[:n])
        else:
            import pybullet_data
            preset['manipulator_file'] = os.path.join(pybullet_data.getDataPath(), preset['manipulator_file'])
            self.initialize_environment(initial_positions_variation_range=variation, visualize=visualize, **preset)

    def run_demo_training(self, demo_type: str, verbose: bool = False, interactive: bool = True,
                          environment: str = 'pybullet', episodes: int = 20, frames: int = 400) -> None:
        """'kuka_training' / 'xarm6_training': preset env + default agent, 20 episodes x 400 frames
        (rl_framework.py:503-598)."""
        old_level = logger.level
        logger.setLevel(10)
        try:
            robot = demo_type[:-len('_training')] if demo_type.endswith('_training') else None
            if robot not in ROBOT_PRESETS:       # the reference knows kuka_training / xarm6_training
                logger.error('Incorrect demo type!')
                return
            if not self._clear_for_demo(interactive):
                return
            variation = list(ROBOT_PRESETS[robot]['training_variation'])
            self._demo_environment(robot, environment, variation, visualize=True)
            self.initialize_naf_agent()
            self.run_training(episodes, frames, verbose=verbose)
            self.delete_environment()
            self.delete_naf_agent()
        finally:
            logger.setLevel(old_level)

    def run_demo_testing(self, demo_type: str, interactive: bool = True, environment: str = 'pybullet',
                         weights_file: Optional[str] = None, episodes: int = 50, frames: int = 750) -> Optional[dict]:
        """'kuka_testing' / 'xarm6_testing': preset env, pretrained weights, 50 x 750-frame test episodes
        (rl_framework.py:600-699). The reference ships demo weights inside its package; pass their path as
        `weights_file` (reference-format .p files load unchanged)."""
        old_level = logger.level
        logger.setLevel(10)
        try:
            robot = demo_type[:-len('_testing')] if demo_type.endswith('_testing') else None
            if robot not in ROBOT_PRESETS:       # the reference knows kuka_testing / xarm6_testing
                logger.error('Incorrect demo type!')
                return None
            if not self._clear_for_demo(interactive):
                return None
            variation = list(ROBOT_PRESETS[robot]['testing_variation'])
            self._demo_environment(robot, environment, variation, visualize=ROBOT_PRESETS[robot]['visualize_testing'])
            self.initialize_naf_agent()
            if weights_file is not None:
                self.load_pretrained_parameters_from_weights_file(weights_file)
            out = self.test_trained_model(episodes, frames)
            self.delete_environment()
            self.delete_naf_agent()
            return out
        finally:
            logger.setLevel(old_level)
