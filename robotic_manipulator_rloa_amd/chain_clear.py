"""ClearLaunch: GoalPoseSolver's optional step (chain_tools.py) — naf_chain_ik_clear between the solve and the clearances, which pushes
the candidates that reach their target and lean on something out of contact in the task's null space (csrc/chain_env.hip;
environment/contact_push.py states the rule). A mix-in, as chain_legs.LegsLaunch is for the demonstration writer: it uses the tool's
library, handle, buffers and chunk, and allocates its own buffers on the first call that asks for the step."""
from __future__ import annotations

from . import _lib
from ._lib import check, ptr, stream_ptr
from .environment.contact_push import clear_defaults, pop_push


class ClearLaunch:
    obstacles = q_work = clear = None      # [chunk][3] per query, [chunk][A] and [chunk][4] per candidate: with avoid_contact only

    def clear_params(self, tolerance: float, margin: float = 0.0, clearance_goal=None, push_iterations=None, push_settle=None,
                     push_max=None, **constants):
        """(naf_chain_ik_params_t with the refinement's trip count, naf_chain_ik_clear_params_t): launch()'s `clear`"""
        p = clear_defaults(margin, clearance_goal, push_iterations, push_settle, push_max)
        return (self.params(p["iterations"], **constants),
                _lib.IkClearParams(int(p["settle"]), float(tolerance), float(p["clearance_goal"]), float(p["push_max"]), self.obstacle_radius))

    def clear_setup(self, constants: dict, tolerance: float, margin: float, orientations=None, approach_directions=None):
        """takes the push's arguments out of solve()'s `constants`: None without avoid_contact, otherwise clear_params, with the
        buffers in place"""
        push = pop_push(constants, orientations, approach_directions)
        if push is None:
            return None
        if self.q_work is None:
            self.obstacles, self.q_work, self.clear = self._zeros(self.chunk, 3), self._zeros(self.chunk, self.A), self._zeros(self.chunk, 4)
        return self.clear_params(tolerance, margin, **push, **constants)

    def load_clear(self, clear, obstacles):
        """a chunk's obstacles[n][3] into the buffer where the step is on; returns `clear` for launch()"""
        if clear is not None:
            self._upload(self.obstacles, obstacles)
        return clear

    def launch_clear(self, n: int, R: int, clear) -> None:
        """naf_chain_ik_clear on the chunk's solved poses, in place: self.q and self.residual become the refined ones"""
        check(self.lib.naf_chain_ik_clear(self._chain_env, ptr(self.targets), ptr(self.obstacles), ptr(self.q), n, R, clear[0], clear[1],
                                          ptr(self.q), ptr(self.q_work), ptr(self.residual), ptr(self.clear), None, None, stream_ptr()),
              "chain_ik_clear")
