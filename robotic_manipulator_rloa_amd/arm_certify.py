"""What ManipulatorFramework.certify_joint_paths does once the facade has looked at the environment: the refusals, then
the certificates of the polylines of a JointPaths — the float64 twin's (environment.edge_certificate.certify_polylines_host), or
the cached device tool's (chain_certify.PolylineCertifier, kind 'polyline_certificates' in arm_planner.ArmPlanner's cache). The
checks shared with the other arm-planning methods are arm_planner's."""
from __future__ import annotations

import numpy as np

from .arm_planner import ArmPlanner, _on_device, _refusing, check_arguments
from .environment.edge_certificate import PathCertificates, certify_polylines_host
from .environment.kinematic import JointPaths, reach_table
from .utils.exceptions import InvalidEnvironmentParameter


def certify_joint_paths(planner: ArmPlanner, paths, obstacles, clearance_margin, resolution, on_device) -> PathCertificates:
    env = planner.env
    if not isinstance(paths, JointPaths) or paths.start is None or paths.goal is None:
        raise InvalidEnvironmentParameter('paths is the JointPaths that plan_joint_paths() returned')
    check_arguments(clearance_margin=clearance_margin, resolution=resolution)
    N, A = np.asarray(paths.start).shape
    if A != env.model.A:
        raise InvalidEnvironmentParameter(f'paths holds poses of {A} joints, the environment\'s arm has {env.model.A}')
    _, _, obstacles, _ = planner.queries(np.zeros((N, 3)), obstacles, None)
    with _refusing():
        reach_table(env.model)                                # an unlimited prismatic joint, by name
    margin, resolution = float(clearance_margin), float(resolution)
    if not _on_device(on_device):
        return certify_polylines_host(env, paths, obstacles, margin, resolution)
    from .chain_certify import PolylineCertifier, PolylineLdsRefusal
    try:
        return planner.tool('polyline_certificates', PolylineCertifier).certify(paths, obstacles, margin, resolution)
    except PolylineLdsRefusal as err:
        raise InvalidEnvironmentParameter(f'certify_joint_paths(): {err} (NAF_CHAIN_ERR_LDS); on_device=False answers this arm '
                                          f'through the float64 twin') from None
