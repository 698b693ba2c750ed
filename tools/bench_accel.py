"""`Accelerate` on a resident plane under both routes, beside a device copy of the output's bytes from the
same run, one JSON line per row (dev tool; needs a GPU).

    python tools/bench_accel.py [--out FILE] [--reps N] [row ...]

Rows: a float32 plane of unit-variance noise (one block of 2^16 samples repeated), resident in HBM, one
block of ``n = length`` rows, trial factors spread evenly over ``|k| n <= 1e-3`` --

    n20x8_a64    (2^20, 8)  x 64 trials: rows of 32 bytes in, 2 KiB out
    n20x64_a16   (2^20, 64) x 16 trials: rows of 256 bytes in, 4 KiB out
    n22x2_a64    (2^22, 2)  x 64 trials: rows of 8 bytes in, 512 bytes out
    chain        (2^20, 8)  x 64 trials: HarmonicSearch(Whiten(LongSpectra(Accelerate(...), n), 128), 64) whole,
                 and its Accelerate stage alone: the share of a full trial that the resampling takes

Every row runs in a child process of its own under a time limit, and the first row that fails ends the
run.  Timed with device events around ``read_device()`` of the whole result (the cache dropped before
every repeat): 2 warm-up reads, then ``--reps`` timed ones; the minimum and the median are reported.  In the
rows that compare, the routes and the copy take turns repeat by repeat after four untimed rounds, as the
first series of a process ran up to 12 % slower than the same route measured later.

  `window_ms`, `direct_ms`: the read under BBT_ACCEL_ROUTE=1 (the window staged in LDS wherever it fits)
      and =2 (global memory only); `auto_ms` under the automatic rule.
  `copy_ms`: a device-to-device copy of the output's bytes; `*_over_copy` the ratios.  A gather that writes
      each byte once has nothing else to be held against."""
import os
import sys

import bench_rows
from bench_rows import events_ms, reread

sys.path.insert(0, bench_rows.ROOT)

ROWS = {
    'n20x8_a64': dict(length=1 << 20, ndm=8, n_acc=64),
    'n20x64_a16': dict(length=1 << 20, ndm=64, n_acc=16),
    'n22x2_a64': dict(length=1 << 22, ndm=2, n_acc=64),
    'chain': dict(length=1 << 20, ndm=8, n_acc=64, chain=True),
}
ROW_LIMIT = 400          # seconds a row may take
RATE = 1e3
REACH = 1e-3             # |k| n at the outermost trials
BURN_IN = 4              # rounds over all routes and the copy before the timed ones


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip, periodicity
    row = ROWS[name]
    length, ndm, n_acc = row['length'], row['ndm'], row['n_acc']
    n = length
    bt.hip.set_device(0)
    rng = np.random.default_rng(7)
    x = np.tile(rng.standard_normal((1 << 16, ndm), dtype=np.float32), (length >> 16, 1))
    plane = bt.DeviceStream(x, bt.Time('2020-01-01T00:00:00'), RATE, samples_per_frame=1 << 14)
    del x
    factors = np.linspace(-REACH, REACH, n_acc) / n
    accelerations = factors * (2. * periodicity.C_LIGHT * RATE)
    values = length * ndm * n_acc
    line = dict(row=name, device=hip.device_name(), length=length, ndm=ndm, n_acc=n_acc, n=n, reach=REACH, reps=reps,
                out_bytes=values * 4)

    def timed(task):
        def read():
            stage = task
            while hasattr(stage, 'invalidate_cache'):             # (every stage of a chain is made again)
                stage.invalidate_cache()
                stage = stage.ih
            task.seek(0)
            task.read_device()
        times = events_ms(read, 2, reps)
        return round(min(times), 3), round(float(np.median(times)), 3)

    acc = bt.Accelerate(plane, accelerations, n)
    line['max_shift'] = acc.max_shift
    plan = hip.AccelPlan(n, ndm, acc.factors)
    whole = plan.info(0, n)
    line.update(rows_per_tile=whole['rows'], lds_bytes=whole['lds_bytes'], auto_route=whole['route'])
    mid = plan.info(n // 2 // whole['rows'] * whole['rows'], whole['rows'])
    line.update(mid_tile_window_rows=mid['window_rows'], mid_tile_fits=mid['fits'])
    plan.close()
    if row.get('chain'):
        sp = bt.LongSpectra(acc, n)
        hs = bt.HarmonicSearch(bt.Whiten(sp, 128), 64)
        line['chain_ms_min'], line['chain_ms_med'] = timed(hs)
        hs.close(), sp.close()
        line['accelerate_ms_min'], line['accelerate_ms_med'] = timed(acc)
        line['accelerate_share'] = round(line['accelerate_ms_min'] / line['chain_ms_min'], 3)
        return line
    # The routes and the copy take turns, repeat by repeat, after a burn-in: measured one after the other,
    # whatever came first was up to 12 % slower than the same route measured third.
    src, dst = hip.DeviceArray((values,), np.float32), hip.DeviceArray((values,), np.float32)
    hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))

    turns = (('auto', '0'), ('window', '1'), ('direct', '2'), ('copy', '0'))
    times = {key: [] for key, _ in turns}
    for r in range(BURN_IN + reps):
        for key, route in turns:
            os.environ['BBT_ACCEL_ROUTE'] = route
            step = (lambda: dst.copy_from_device(src)) if key == 'copy' else (lambda: reread(acc))
            t = events_ms(step, 2 if r == 0 else 0, 1)
            if r >= BURN_IN:
                times[key] += t
    os.environ['BBT_ACCEL_ROUTE'] = '0'
    acc.close()
    del src, dst
    for key, _ in turns:
        line[key + '_ms'], line[key + '_ms_med'] = round(min(times[key]), 3), round(float(np.median(times[key])), 3)
    for key in ('auto', 'window', 'direct'):
        line[key + '_over_copy'] = round(line[key + '_ms'] / line['copy_ms'], 2)
    line['copy_tb_per_s'] = round(values * 8 / line['copy_ms'] / 1e9, 3)
    return line


if __name__ == '__main__':
    sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'accel_bench.jsonl'))
