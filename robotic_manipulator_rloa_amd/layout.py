"""Where the parameters of one NAF network sit inside the learner's flat buffers (see learner.py): host-side integers
only — chain_plan.py and learner.py both build on it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import torch

from . import _lib


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


@dataclass(frozen=True)
class Segment:
    offset: int
    shape: Tuple[int, ...]

    @property
    def numel(self) -> int:
        n = 1
        for s in self.shape:
            n *= s
        return n


BB_MAX_STATE = 32      # the row-split chain: layer 1's K (csrc/big_batch.hip, BB_MAX_K4)
BB_MAX_JOINTS = 11     # ... and the fused layer-2 launch's heads tile (FK_MAX_A)
NATIVE_LAYER = 256     # the width the fused kernels are built for (rl_framework.py's presets; csrc/big_batch.hip, step_path.hip)


class NetLayout:
    """Where each parameter of one NAF network sits inside its flat buffer (units: floats).
    Segments start on 64-float (256-B) boundaries; the gaps and the pad rows/columns of Wh hold zeros, receive
    zero gradients and therefore stay zero under Adam.

    layer_size below 256 (the reference takes any; its own agent test builds 128): with pad_layer the network is STORED as a
    256-wide one whose units beyond layer_size have zero weights, zero biases and zero BatchNorm scale / shift — `H` (what every
    kernel sees) is 256, `H_ref` (what state_dict() shows and load_state_dict() takes) is layer_size. Such a unit's pre-activation is
    0 for every sample, its normalised value 0, its activation ReLU(0 * 0 + 0) = 0; nothing downstream multiplies it with anything
    but a zero weight, so every gradient it receives or passes on is 0 and Adam (m = v = 0) leaves it where it is: the padded network
    computes the narrow one's numbers, term for term, with exact zeros appended to its sums — and runs the kernels the presets run."""

    def __init__(self, state_size: int, action_size: int, layer_size: int, pad_layer: bool = True):
        if not (1 <= action_size <= 64):
            raise ValueError("action_size must be in 1..64 (one sample per 8- or 16-lane group in the fused head kernels, per 16-, "
                             "32- or 64-lane group in the stand-alone ones: a wavefront has 64 lanes)")
        self.H_ref = int(layer_size)
        self.S, self.A = state_size, action_size
        # (round 6: widths in (256, 512) likewise stored as 512 — the row-split chain runs 512 columns as two 256-column halves)
        self.H = (NATIVE_LAYER if (pad_layer and 0 < layer_size < NATIVE_LAYER) else
                  2 * NATIVE_LAYER if (pad_layer and NATIVE_LAYER < layer_size < 2 * NATIVE_LAYER) else int(layer_size))
        self.T = action_size * (action_size + 1) // 2
        self.NH = self.A + self.T + 1                  # [mu | l | V]
        self.NHP = _round_up(self.NH, 16)              # heads row stride (ldh): whole 16-wide MFMA tiles
        self.HP = self.H + 16                          # activations: H features | 1.0 | 15 zeros (K % 16 == 0)
        self.seg: Dict[str, Segment] = {}
        off = 0
        for name, shape in (("W1", (self.H, self.S)), ("b1", (self.H,)), ("g1", (self.H,)), ("be1", (self.H,)),
                            ("W2", (self.H, self.H)), ("b2", (self.H,)), ("g2", (self.H,)), ("be2", (self.H,)),
                            ("Wh", (self.NHP, self.HP))):
            self.seg[name] = Segment(off, shape)
            off = _round_up(off + self.seg[name].numel, 64)
        self.P = off
        self.row_floats = _lib.load().naf_replay_row_floats(self.S, self.A)              # ring rows (256 B)
        self.batch_row_floats = _lib.load().naf_replay_batch_row_floats(self.S, self.A)  # gathered minibatch rows
        # offsets inside a transition row
        self.off_u = self.S
        self.off_r = self.S + self.A
        self.off_s2 = _lib.load().naf_replay_row_off_next_state(self.S, self.A)   # 16-B aligned
        self.off_d = self.off_s2 + self.S

    @property
    def ends_with_wh(self) -> bool:
        """Wh is the last segment and nothing pads the buffer behind it: what the gradient exchange's push of [Wh, P) and its
        merged form (csrc/big_batch.hip, bb_finish_exchange) need."""
        return self.seg["Wh"].offset + self.seg["Wh"].numel == self.P

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        s = self.seg[name]
        return flat[s.offset:s.offset + s.numel].view(*s.shape)

    def n_ref_params(self) -> int:
        """Number of parameters of the reference module (79,644 at S=21, A=6, H=256)."""
        h = self.H_ref
        return h * self.S + h * h + 6 * h + self.NH * (h + 1)

    # ---- mapping to the reference's state_dict keys (naf_neural_network.py:37-54) -------------------------
    def param_views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """the reference's tensors, in its shapes: views of the stored ones (of their first layer_size units where the layer is
        stored padded; the heads' bias column is column H of Wh)"""
        A, T, H, h = self.A, self.T, self.H, self.H_ref
        Wh = self.view(flat, "Wh")
        return {
            "input_layer.weight": self.view(flat, "W1")[:h], "input_layer.bias": self.view(flat, "b1")[:h],
            "bn1.weight": self.view(flat, "g1")[:h], "bn1.bias": self.view(flat, "be1")[:h],
            "hidden_layer.weight": self.view(flat, "W2")[:h, :h], "hidden_layer.bias": self.view(flat, "b2")[:h],
            "bn2.weight": self.view(flat, "g2")[:h], "bn2.bias": self.view(flat, "be2")[:h],
            "action_values.weight": Wh[0:A, 0:h], "action_values.bias": Wh[0:A, H],
            "value.weight": Wh[A + T:A + T + 1, 0:h], "value.bias": Wh[A + T:A + T + 1, H],
            "matrix_entries.weight": Wh[A:A + T, 0:h], "matrix_entries.bias": Wh[A:A + T, H],
        }
