"""Argument checks of the normal-stream entry points of the C ABI (no GPU needed: they fail
before anything is queued)."""
import ctypes as C

import numpy as np

from baseband_tasks_amd import hip


def test_philox_normal_rejects_bad_arguments():
    lib = hip.lib()
    need = C.c_int64()
    assert lib.bbt_philox_normal_work(1, 4096, None) != 0 and b'null' in lib.bbt_last_error()
    assert lib.bbt_philox_normal_work(0, 4096, C.byref(need)) != 0 and b'bad sizes' in lib.bbt_last_error()
    assert lib.bbt_philox_normal_work(70000, 4096, C.byref(need)) != 0
    assert lib.bbt_philox_normal_work(1, 4094, C.byref(need)) != 0 and b'bad sizes' in lib.bbt_last_error()
    assert lib.bbt_philox_normal_work(2, 4100, C.byref(need)) == 0
    # 2 frames x 5 tiles: counters, totals, flags (6 x 8 bytes a frame), 8 + 32 bytes a tile
    assert need.value == 2 * 48 + 10 * 40
    key = np.zeros(2, np.uint64)
    ctr = np.zeros((2, 4), np.uint64)
    totals = (C.c_int64 * 2)()
    flags = (C.c_int64 * 2)()
    fake = 1 << 20                                         # an address that is never touched
    args = dict(key=key.ctypes.data, ctr=ctr.ctypes.data, n_frame=2, n=3000, n_words=4100, guard=2.0**-46,
                out=fake, stride=3000, work=fake, work_bytes=need.value, totals=totals, flags=flags)

    def call(**change):
        a = dict(args, **change)
        return lib.bbt_philox_normal(a['key'], a['ctr'], a['n_frame'], a['n'], a['n_words'], a['guard'], a['out'],
                                     a['stride'], a['work'], a['work_bytes'], a['totals'], a['flags'], None)

    for name in ('key', 'ctr', 'out', 'work', 'totals', 'flags'):
        assert call(**{name: None}) != 0 and b'null argument' in lib.bbt_last_error(), name
    assert call(n=0) != 0 and b'frame length' in lib.bbt_last_error()
    assert call(n=3001) != 0 and b'stride' in lib.bbt_last_error()
    assert call(n_words=4098) != 0 and b'bad sizes' in lib.bbt_last_error()
    assert call(guard=-1.0) != 0 and b'guard' in lib.bbt_last_error()
    assert call(work_bytes=need.value - 1) != 0 and b'needed' in lib.bbt_last_error()
    assert call(work=fake + 8) != 0 and b'aligned' in lib.bbt_last_error()
    assert call(out=fake + 2) != 0 and b'aligned' in lib.bbt_last_error()
