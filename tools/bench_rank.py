"""`RobustStandardize` beside `Standardize` and `MedianWhiten` beside `Whiten` on resident arrays, the
routes of the selection kernel beside each other, and a device-to-device copy, all from the same run:
one JSON line per row (dev tool; needs a GPU).

    python tools/bench_rank.py [--out FILE] [--reps N] [row ...]

Rows: `std_256`, `std_4096`, `std_65536`: a float32 noise plane of (2^16, 512) resident in HBM,
standardized in blocks of 256, 4096 and 65536 samples; `whiten_128`: a (64, 8193, 512) stack of
exponential spectra whitened in blocks of 128 bins.  Every row runs in a child process of its own under
a time limit, and the first row that fails ends the run.

Timed with device events around ``read_device()`` of the whole result (the cache dropped before every
read).  The candidates of a row TAKE TURNS -- copy, the mean-based task, the median-based task on the
automatic route, on the other route where both can run (BBT_RANK_ROUTE is read at every call), and on
the global route with 64-wide tiles -- two warm-up turns, then ``--reps`` timed ones; the minimum of
each is reported, with its ratio to the mean-based task (`*_over_plain`) and to the copy
(`*_over_copy`).  `route`, `digit` and `width` say what the automatic rule took."""
import os
import sys

import bench_rows
from bench_rows import reread, take_turns

sys.path.insert(0, bench_rows.ROOT)

ROWS = {
    'std_256': dict(kind='std', shape=(1 << 16, 512), block=256),
    'std_4096': dict(kind='std', shape=(1 << 16, 512), block=4096),
    'std_65536': dict(kind='std', shape=(1 << 16, 512), block=65536),
    'whiten_128': dict(kind='whiten', shape=(64, 8193, 512), block=128),
}
ROW_LIMIT = 300          # seconds a row may take
RATE = 1e4
WARM = 2


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip
    row = ROWS[name]
    shape, block = row['shape'], row['block']
    for key in ('BBT_RANK_ROUTE', 'BBT_RANK_DIGIT', 'BBT_RANK_WIDTH'):
        os.environ.pop(key, None)
    bt.hip.set_device(0)
    rng = np.random.default_rng(7)
    t0 = bt.Time('2020-01-01T00:00:00')
    if row['kind'] == 'std':
        x = rng.standard_normal(shape, dtype=np.float32)
        ih = bt.DeviceStream(x, t0, RATE, samples_per_frame=shape[0])
        plain = bt.Standardize(ih, block, samples_per_frame=shape[0])
        robust = bt.RobustStandardize(ih, block, samples_per_frame=shape[0])
        info = hip.rank_info(1, shape[0], shape[1], block, 0)
    else:
        x = rng.standard_exponential(shape, dtype=np.float32)
        ih = bt.DeviceStream(x, t0, RATE, samples_per_frame=shape[0])
        plain = bt.Whiten(ih, block, samples_per_frame=shape[0])
        robust = bt.MedianWhiten(ih, block, samples_per_frame=shape[0])
        info = hip.rank_info(shape[0], shape[1], shape[2], block, 1)
    words = int(np.prod(shape))
    del x
    src, dst = hip.DeviceArray((words,), np.float32), hip.DeviceArray((words,), np.float32)
    hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))

    def read(task, env):
        def step():
            for key in ('BBT_RANK_ROUTE', 'BBT_RANK_WIDTH'):
                os.environ.pop(key, None)
            os.environ.update(env)
            reread(task)
        return step

    candidates = {'copy': lambda: dst.copy_from_device(src), 'plain': read(plain, {}), 'auto': read(robust, {})}
    if info['route'] == 'lds':
        candidates['global'] = read(robust, dict(BBT_RANK_ROUTE='global'))
    candidates['global_w64'] = read(robust, dict(BBT_RANK_ROUTE='global', BBT_RANK_WIDTH='64'))
    times = take_turns(candidates, WARM, reps)
    line = dict(row=name, device=hip.device_name(), shape=list(shape), block=block, reps=reps, bytes=words * 4,
                route=info['route'], digit=info['digit'], width=info['width'], lds_bytes=info['lds_bytes'])
    for key, values in times.items():
        line[f'{key}_ms'] = round(min(values), 3)
        line[f'{key}_ms_med'] = round(float(np.median(values)), 3)
    for key in candidates:
        if key not in ('copy', 'plain'):
            line[f'{key}_over_plain'] = round(line[f'{key}_ms'] / line['plain_ms'], 2)
            line[f'{key}_over_copy'] = round(line[f'{key}_ms'] / line['copy_ms'], 2)
    line['plain_over_copy'] = round(line['plain_ms'] / line['copy_ms'], 2)
    return line


if __name__ == '__main__':
    sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'rank_bench.jsonl'))
