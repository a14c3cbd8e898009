"""Guard bands around every per-environment buffer: what a kernel writes BESIDE its rows.

``GuardRegistry.zeros / ones / full`` have the call shape of the torch functions of the same name.  Each call allocates ONE
uint8 buffer -- front guard, payload, back guard -- fills all of it with 0xFF bytes and returns the payload as a contiguous
view with the requested dtype, shape and fill value.  0xFF reads as NaN in float64 and float32, -1 as int32, 255 as uint8:
a stray READ poisons what it feeds, a stray WRITE changes a guard byte.  A guard is at least 64 rows of its buffer (a row:
everything behind the leading dimension; 64 rows cover every idle lane of a last block writing its own row), rounded up to
a multiple of 512 bytes, which keeps the payload at the alignment a torch allocation has.

``with registry.guarding():`` routes ``torch.zeros``, ``torch.ones`` and ``torch.full`` through the registry -- the three
calls by which envs/anm_env.py, envs/mixed.py, simulator.py and agents/mpc.py allocate every buffer a kernel writes.
``registry.check()`` returns the buffers whose guards are not 0xFF throughout: byte comparison, no tolerance."""
import contextlib

import numpy as np
import torch

GUARD_ROWS = 64
GUARD_ALIGN = 512
FILL = 0xFF

# the real function, bound once: the registry itself allocates through it also while a `guarding()` block is open
_FULL = torch.full


def _shape_of(size):
    """torch's `*size`: zeros(3), zeros(3, 4), zeros((3, 4)), zeros(torch.Size(...))"""
    if len(size) == 1 and not isinstance(size[0], (int, np.integer)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def guard_bytes(shape, itemsize):
    """bytes of ONE guard of a buffer of this shape: >= 64 rows, a multiple of 512, never 0"""
    row = int(np.prod(shape[1:], dtype=np.int64)) * itemsize
    return max(GUARD_ALIGN, -(-GUARD_ROWS * row // GUARD_ALIGN) * GUARD_ALIGN)


class Guarded:
    """one allocation: `big` = front guard | payload | back guard (uint8), `payload` the typed view handed out"""

    def __init__(self, big, payload, guard, nbytes):
        self.big, self.payload, self.guard, self.nbytes = big, payload, guard, nbytes

    @property
    def shape(self):
        return tuple(self.payload.shape)

    @property
    def dtype(self):
        return self.payload.dtype


class GuardRegistry:
    def __init__(self):
        self.buffers = []

    # ---- the allocator ---------------------------------------------------------------------------------------------------
    def alloc(self, shape, fill, dtype=None, device=None):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        shape = _shape_of((shape,))
        itemsize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        g = guard_bytes(shape, itemsize)
        big = _FULL((g + nbytes + g,), FILL, dtype=torch.uint8, device=device)
        payload = big[g:g + nbytes].view(dtype).view(shape)
        payload.fill_(fill)
        assert payload.is_contiguous() and payload.data_ptr() == big.data_ptr() + g
        self.buffers.append(Guarded(big, payload, g, nbytes))
        return payload

    def zeros(self, *size, dtype=None, device=None):
        return self.alloc(_shape_of(size), 0, dtype, device)

    def ones(self, *size, dtype=None, device=None):
        return self.alloc(_shape_of(size), 1, dtype, device)

    def full(self, size, fill_value, *, dtype=None, device=None):
        if dtype is None:   # torch.full infers it from the value
            dtype = torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int) else None
        return self.alloc(_shape_of((size,)), fill_value, dtype, device)

    def like(self, t):
        """a guarded copy of a tensor the test brings (actions, init_state, masks ...)"""
        out = self.alloc(tuple(t.shape), 0, t.dtype, t.device)
        out.copy_(t)
        return out

    # ---- routing the three torch calls -------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def guarding(self):
        """torch.zeros / torch.ones / torch.full allocate through this registry inside the block (what they had before is
        put back on the way out, also on an exception).  Keyword arguments the registry does not know are refused, not
        ignored: a buffer that silently stayed unguarded would be a hole in the net."""
        before = torch.zeros, torch.ones, torch.full
        torch.zeros, torch.ones, torch.full = self.zeros, self.ones, self.full
        try:
            yield self
        finally:
            torch.zeros, torch.ones, torch.full = before

    # ---- the check -----------------------------------------------------------------------------------------------------------
    def check(self):
        """-> [(index, shape, dtype, offset)] of the buffers with a changed guard byte; `offset` is the first changed byte
        relative to the payload's first byte (negative: the front guard; >= the payload's bytes: the back guard)."""
        by_device = {}
        for i, b in enumerate(self.buffers):   # one flag per buffer, one copy to the host per device
            flag = (b.big[:b.guard] != FILL).any() | (b.big[b.guard + b.nbytes:] != FILL).any()
            by_device.setdefault(b.big.device, []).append((i, flag))
        hit = []
        for pairs in by_device.values():
            flags = torch.stack([f for _, f in pairs]).cpu().numpy()
            hit += [pairs[k][0] for k in np.nonzero(flags)[0]]
        bad = []
        for i in sorted(hit):
            b = self.buffers[i]
            front = torch.nonzero(b.big[:b.guard] != FILL)
            back = torch.nonzero(b.big[b.guard + b.nbytes:] != FILL)
            off = int(front[0]) - b.guard if front.numel() else b.nbytes + int(back[0])
            bad.append((int(i), b.shape, b.dtype, off))
        return bad

    def assert_intact(self, where):
        bad = self.check()
        assert not bad, "%s: written outside the rows -- (buffer, shape, dtype, first byte offset): %r" % (where, bad)
