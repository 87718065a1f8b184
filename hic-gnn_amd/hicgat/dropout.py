"""The state behind feature dropout on the HIP path: a seed and a step count on the device.

The keep mask is a pure function of (seed, step, site, row, column) (include/hicgat.h, DESIGN.md
"Feature dropout"), so nothing random is drawn on the host: a training forward advances the count
once (``advance``: one tiny launch, first in the forward) and every dropout site of that forward
reads it from the device.  A captured step therefore replays as the next step, with the bits an
eager step would give.
"""
import torch

from . import _lib, kernels

_U64 = (1 << 64) - 1


def check_p(p):
    """The drop probability as a float in [0, 1) (ValueError otherwise; NaN included)."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must satisfy 0 <= p < 1, got {p}")
    return p


class DropoutState:
    """``seed`` (default ``torch.initial_seed()``: read, not drawn, so seeded initial weights are
    unchanged) and the count of training forwards so far, an int64 on ``device`` starting at 0 (the
    first training forward runs with step 1).  ``p``: the probability the owning model's sites use
    (the model sets it; None for a bare state)."""

    def __init__(self, device, seed=None, p=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.HicgatUnavailable(f"DropoutState needs a CUDA (HIP) device; got {device}")
        self._p = None if p is None else check_p(p)
        self.seed = (torch.initial_seed() if seed is None else int(seed)) & _U64
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DropoutState must be created before the step is captured (its counter would be "
                               "re-zeroed by every replay): run one eager training forward first")
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)

    @property
    def p(self):
        return self._p

    @p.setter
    def p(self, value):
        self._p = None if value is None else check_p(value)

    @property
    def device(self):
        return self.counter.device

    def advance(self):
        """counter += 1 on the current stream (the first launch of a training forward)."""
        kernels.default().dropout_advance(self.counter)

    @property
    def step(self):
        """The count, read back (a host sync)."""
        return int(self.counter.item())

    def reset(self, seed=None, step=0):
        if seed is not None:
            self.seed = int(seed) & _U64
        self.counter.fill_(int(step))
