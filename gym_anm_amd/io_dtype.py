"""Float32 policy-facing I/O (``BatchedANMEnv(io_dtype=torch.float32)``; ``anm_model_set_io`` in the C ABI): the
specification the kernels follow (csrc/anm_env_ops.hpp: ``EnvIO::io32``, ``io_store``, the ``IO32`` instantiations of the
coalesced-row step; the lane-group kernels carry a float32 instance of their output sections).  Like ``rng.py`` and
``episode.py`` this text is normative: the kernels are tested against it bit for bit.

The mode changes the number format of three arrays and nothing else.

1. Action.  The kernel reads ``float action[E, action_dim]`` and widens every entry to double, which is exact.  A float32-mode
   step with actions ``a32`` therefore equals the float64-mode step with ``a32.double()`` bit for bit in every float64
   quantity: ``state``, ``soc``, ``e_loss``, ``penalty``, ``terminated``, ``truncated``, ``timestep``, ``reset_count``,
   ``nr_iters`` and all episode statistics (which accumulate the float64 reward).
2. Observation.  ``obs32 = (float) obs64``: ONE round-to-nearest-even conversion of the value the float64 mode would have
   written, after the clip (:func:`to_float32`; subnormals are kept and overflow goes to +-inf, as ``tensor.to(torch.float32)``
   does).  This holds for the ``"state"`` form, for the list form gathered in the kernel, for the zero rows of terminated
   environments and for the rows an in-kernel autoreset writes.
3. Reward.  ``reward32 = (float) reward64``, the same single rounding.  ``e_loss``, ``penalty``, ``state``, ``soc`` and the
   episode buffers stay float64: they are the environment's own state and its diagnostics.
4. Spaces.  ``observation_space`` is a float32 ``Box`` whose bounds are rounded to nearest (:func:`observation_bounds32`):
   the conversion is monotone, so ``clip(x, lo, hi)`` rounded lies inside it.  ``action_space`` is a float32 ``Box`` whose
   bounds are rounded INWARD (:func:`action_bounds32`): the largest float32 <= ``high`` and the smallest float32 >= ``low``,
   so that every float32 point of the ``Box`` lies in the float64 ``Box`` the reference defines.  ``check_actions`` compares
   against these bounds in float32.
5. ``reset()`` returns float32 observations under rule 2.  The reset kernel writes the ``"state"`` form in float32 itself;
   the list form at reset is gathered in float64 and cast once on the host side of the launch (``reset()`` is not the hot
   path).
6. The state row is always written: it has no float64 twin in ``obs`` (``anm_model_bind_state_same`` is not used).

Not served (refused, not ignored): a backend other than the GPU library, parameter classes (``variants=``), batch views and
``MixedBatchedANMEnv``, a list-form observation that is not gathered inside the step kernel, ``track_full`` without such a
list, and any dtype other than float32 / float64.
"""

from __future__ import annotations

import numpy as np
import torch

from . import errors as E

_F32_NAMES = {"float32": torch.float32, "float64": torch.float64}


def check_io_dtype(io_dtype):
    """``None`` / ``torch.float64`` (today's interface) or ``torch.float32``; NumPy's two dtypes are taken for them.  Anything
    else is an ``ArgsError``."""
    if io_dtype is None:
        return torch.float64
    if isinstance(io_dtype, torch.dtype):
        if io_dtype in (torch.float32, torch.float64):
            return io_dtype
    else:
        try:
            name = np.dtype(io_dtype).name
        except TypeError:
            name = None
        if name in _F32_NAMES and not isinstance(io_dtype, str):
            return _F32_NAMES[name]
    raise E.ArgsError("The argument io_dtype is %r but should be torch.float32 or torch.float64." % (io_dtype,))


def to_float32(x):
    """Rule 2 / 3 on a float64 tensor or array: one round-to-nearest-even conversion."""
    if isinstance(x, torch.Tensor):
        return x.to(torch.float32)
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def observation_bounds32(low, high):
    """Rule 4: float32 bounds of the observation ``Box``, each rounded to nearest."""
    return to_float32(low), to_float32(high)


def action_bounds32(low, high):
    """Rule 4: float32 bounds of the action ``Box``, rounded inward (the smallest float32 >= low, the largest <= high)."""
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    lo, hi = to_float32(low), to_float32(high)
    lo = np.where(lo.astype(np.float64) < low, np.nextafter(lo, np.float32(np.inf)), lo)
    hi = np.where(hi.astype(np.float64) > high, np.nextafter(hi, np.float32(-np.inf)), hi)
    return lo.astype(np.float32), hi.astype(np.float32)
