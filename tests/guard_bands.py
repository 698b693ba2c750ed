"""Guarded device arrays for test_guard_bands_gpu.py: a payload between two bands of poison inside ONE
allocation, so that a kernel's store or load beyond the array it was handed lands in memory this module
owns and checks, not in a neighbour's block of the pool.

    | front words of poison | payload | back words of poison |          (a word is 4 bytes)

The payload is a plain view, ``hip.DeviceArray(shape, dtype, ptr=base.ptr + 4 * front, owner=base)``: the
entry points see an array like any other.  Each band holds at least one whole leading-axis row of the
payload plus `PAD` words, so that a store a full row beyond either end is still caught.

TWO OFFSETS.  ``skew`` is the payload's address modulo 16: 0, the alignment every array of the pool has,
or 4, the least the entry points accept; three of them (Accelerate, SpectralKurtosis / Excise, Modulate)
pick another instantiation from it.  complex64 arrays of the spectral-kurtosis entry points, which ask
for pointers aligned to their elements, take 8 instead.  The address is asserted, not assumed.  Any skew
below 16 that is a multiple of the item size (of 4 for items wider than that) is taken: 1 and 2 for the
one- and two-byte elements of the gather plans (test_shaping_guard_gpu.py).  The front band's pattern ends
with a whole word at the payload's first byte, whatever the skew.

TWO POISONS, one per run for all its bands: the quiet NaN 0x7fc0beef and +inf.  The searches leave a NaN
out of their total order, so a stray NaN summand can lose silently; a stray +inf wins its block or spoils
its mean.  uint8 arrays take the byte 0xa5.  Outputs are poisoned throughout, so that a cell the kernel
never writes shows in the comparison with the twin.  `load` asserts that the payload does not hold the
poison word, or holds it exactly as often as the caller says its data plant it."""
import numpy as np

from baseband_tasks_amd import hip

NAN_POISON = 0x7fc0beef
INF_POISON = 0x7f800000
POISONS = {'nan': NAN_POISON, 'inf': INF_POISON}
BYTE_POISON = 0xa5
#: words of a band beyond one leading-axis row
PAD = 64
#: the payload's address modulo 16
SKEWS = (0, 4)


def _poison_bytes(poison, dtype, count):
    """``count`` bytes of the band pattern for an array of ``dtype``, starting at a word boundary."""
    if np.dtype(dtype).itemsize == 1:
        return np.full(count, BYTE_POISON, np.uint8)
    return np.resize(np.array([poison], '<u4').view(np.uint8), count)


class Guarded:
    """One allocation: ``front`` words of poison, a poisoned payload of ``shape`` and ``dtype``, ``back`` words
    of poison.  ``array`` is the payload's view.  ``skew``: the payload's address modulo 16, a multiple of the
    item size (of 4 for wider items); ``front`` counts the front band's whole words, ``front_bytes`` all of it."""

    def __init__(self, shape, dtype, poison, skew=0):
        shape = tuple(int(d) for d in shape)
        self.dtype = np.dtype(dtype)
        assert poison in POISONS.values() and len(shape) >= 1
        assert 0 <= skew < 16 and skew % min(self.dtype.itemsize, 4) == 0, (skew, self.dtype)
        self.poison, self.skew = poison, skew
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * self.dtype.itemsize
        self.row_bytes = self.nbytes // shape[0] if shape[0] else 0
        band = -(-self.row_bytes // 4) + PAD
        # the front band: at least `band` words, and the payload skew bytes past a multiple of 16
        self.front = -(-band // 4) * 4 + skew // 4
        self.front_bytes = 4 * self.front + skew % 4
        # the back band begins at the word boundary at or after the payload's end
        self.tail = -self.nbytes % 4
        self.back = band
        total = self.front_bytes + self.nbytes + self.tail + 4 * self.back
        self.base = hip.DeviceArray((total,), np.uint8)
        assert self.base.ptr % 16 == 0, 'the pool hands out 16-byte aligned blocks'
        # (the front band's pattern is anchored at its end: the last four bytes before the payload are one word)
        self._fill = np.concatenate([_poison_bytes(poison, np.uint32, 4 * self.front + 4)[4 - skew % 4:],
                                     _poison_bytes(poison, self.dtype, self.nbytes),
                                     _poison_bytes(poison, self.dtype, self.tail),
                                     _poison_bytes(poison, np.uint32, 4 * self.back)])
        if self.dtype.itemsize == 1:
            self._fill[:] = BYTE_POISON
        self.base.copy_from_host(self._fill)
        self.array = hip.DeviceArray(shape, self.dtype, ptr=self.base.ptr + self.front_bytes, owner=self.base)
        # the property under test, stated
        assert self.array.ptr % 16 == skew and self.array.nbytes == self.nbytes
        assert 4 * min(self.front, self.back) >= self.row_bytes + 4 * PAD

    @classmethod
    def load(cls, host, poison, skew=0, planted=0):
        """A guarded copy of ``host``.  ``planted``: how often the data hold the poison word on purpose (None:
        they plant it, `accel_cases.SPECIALS`, and the caller does not count); anything else is refused, since
        a stray poison could then pass for data."""
        host = np.ascontiguousarray(host)
        g = cls(host.shape, host.dtype, poison, skew)
        if host.dtype.itemsize == 1:
            found = int(np.count_nonzero(host.view(np.uint8) == BYTE_POISON))
        else:
            # (the payload's whole words; two-byte data may end with half a one)
            words = host.reshape(-1).view(np.uint8)[:host.nbytes // 4 * 4].view(np.uint32)
            found = int(np.count_nonzero(words == poison))
        assert planted is None or found == planted, f'the payload holds the poison {poison:#x} {found} times'
        g.array.copy_from_host(host)
        return g

    def check(self, what=''):
        """Downloads the whole allocation, asserts that both bands are word for word the poison -- naming the
        first touched word relative to the payload, in words and in leading-axis rows -- and returns the
        payload."""
        got = self.base.to_host()
        begin, end = self.front_bytes, self.front_bytes + self.nbytes
        band = np.ones(got.shape[0], bool)
        band[begin:end] = False
        touched = np.flatnonzero(band & (got != self._fill))
        if touched.size:
            at = int(touched[0]) - begin
            side = 'before the payload' if at < 0 else 'past the payload'
            rows = f', row {at // self.row_bytes}' if self.row_bytes else ''
            word = bytes(got[begin + at // 4 * 4:begin + at // 4 * 4 + 4]).hex()
            raise AssertionError(f'{what}: guard band touched {side}: word {at // 4}{rows} of a payload of '
                                 f'{self.nbytes // 4} words ({touched.size} bytes touched in all; the word now holds '
                                 f'{word}, bytes in memory order; poison {self.poison:#x})')
        return got[begin:end].copy().view(self.dtype).reshape(self.array.shape)


def check_all(guarded, what=''):
    """`Guarded.check` of every array of a run (None entries skipped); the payloads in the same order."""
    return [None if g is None else g.check(f'{what} [{i}]') for i, g in enumerate(guarded)]
