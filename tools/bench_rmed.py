"""`Detrend` on resident planes beside `Standardize`, `RobustStandardize` and a device-to-device copy, its
two selection methods beside each other, all from the same run: one JSON line per row (dev tool; needs a
GPU).

    python tools/bench_rmed.py [--out FILE] [--reps N] [row ...]

Rows: `w65_s16`, `w129_s8`, `w129_s1`: a float32 noise plane of (2^20, 512) resident in HBM, detrended with
a window of 65 points of the series scrunched by 16, of 129 by 8 and of 129 samples; `w1023_s1`: a plane
of (2^18, 64) under the widest window.  Every row runs in a child process of its own under a time limit,
and the first row that fails ends the run.

Timed with device events around ``read_device()`` of the whole result (the cache dropped before every
read).  The candidates of a row TAKE TURNS -- copy, `Standardize(..., 4096)`, `RobustStandardize(..., 4096)`,
`Detrend` on the automatic method (the walk) and on the fresh radix descent (BBT_RMED_SELECT is read at
every call) -- two warm-up turns, then ``--reps`` timed ones; the minimum of each is reported, with its
ratio to the copy (`*_over_copy`) and to `RobustStandardize` (`*_over_robust`).  `method`, `tile` and `rows`
say what the automatic rule took."""
import os
import sys

import bench_rows
from bench_rows import reread, take_turns

sys.path.insert(0, bench_rows.ROOT)

ROWS = {
    'w65_s16': dict(shape=(1 << 20, 512), width=65, scrunch=16),
    'w129_s8': dict(shape=(1 << 20, 512), width=129, scrunch=8),
    'w129_s1': dict(shape=(1 << 20, 512), width=129, scrunch=1),
    'w1023_s1': dict(shape=(1 << 18, 64), width=1023, scrunch=1),
}
ROW_LIMIT = 300          # seconds a row may take
RATE = 1e4
WARM = 2
BLOCK = 4096


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip
    row = ROWS[name]
    shape, width, scrunch = row['shape'], row['width'], row['scrunch']
    os.environ.pop('BBT_RMED_SELECT', None)
    bt.hip.set_device(0)
    rng = np.random.default_rng(7)
    t0 = bt.Time('2020-01-01T00:00:00')
    x = rng.standard_normal(shape, dtype=np.float32)
    ih = bt.DeviceStream(x, t0, RATE, samples_per_frame=shape[0])
    plain = bt.Standardize(ih, BLOCK, samples_per_frame=shape[0])
    robust = bt.RobustStandardize(ih, BLOCK, samples_per_frame=shape[0])
    detrend = bt.Detrend(ih, width, scrunch, samples_per_frame=shape[0])
    chunk = min(detrend._chunk_size(), shape[0])
    info = hip.rmed_info(width, scrunch, shape[1], shape[0] // scrunch, 0, chunk)
    words = int(np.prod(shape))
    del x
    src, dst = hip.DeviceArray((words,), np.float32), hip.DeviceArray((words,), np.float32)
    hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))

    def read(task, env):
        def step():
            os.environ.pop('BBT_RMED_SELECT', None)
            os.environ.update(env)
            reread(task)
        return step

    candidates = {'copy': lambda: dst.copy_from_device(src), 'plain': read(plain, {}), 'robust': read(robust, {}),
                  'walk': read(detrend, {}), 'radix': read(detrend, dict(BBT_RMED_SELECT='1'))}
    times = take_turns(candidates, WARM, reps)
    line = dict(row=name, device=hip.device_name(), shape=list(shape), width=width, scrunch=scrunch, block=BLOCK, reps=reps,
                bytes=words * 4, chunk=chunk, method=info['method'], tile=info['tile'], rows=info['rows'],
                lds_bytes=info['lds_bytes'], scratch_bytes=info['scratch_bytes'])
    for key, values in times.items():
        line[f'{key}_ms'] = round(min(values), 3)
        line[f'{key}_ms_med'] = round(float(np.median(values)), 3)
    for key in candidates:
        if key != 'copy':
            line[f'{key}_over_copy'] = round(line[f'{key}_ms'] / line['copy_ms'], 2)
        if key in ('walk', 'radix'):
            line[f'{key}_over_robust'] = round(line[f'{key}_ms'] / line['robust_ms'], 2)
    return line


if __name__ == '__main__':
    sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'rmed_bench.jsonl'))
