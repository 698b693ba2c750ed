"""`LongSpectra` on a resident plane against two yardsticks from the same run, one JSON line per row
(dev tool; needs a GPU).

    python tools/bench_lspec.py [--out FILE] [--reps N] [row ...]

Rows: a float32 plane of unit-variance noise (what `Standardize` hands on; one block of 2^16 samples
repeated, which costs the host less and the device the same), resident in HBM --

    n20          (2^20, 512), one transform of 2^20 per trial
    n22          (2^22, 256), one transform of 2^22 per trial
    n15_stack32  (2^20, 512), 32 stacked transforms of 2^15 per trial

Every row runs in a child process of its own under a time limit, and the first row that fails ends the
run.  Timed with device events around ``read_device()`` of the whole result (the cache dropped before
every repeat): 2 warm-up reads, then ``--reps`` timed ones; the minimum and the median are reported.

  `copy_ms`: a device-to-device copy of the plane's bytes.
  `short_ms`: what the short route makes of the same plane, ``fluctuation_spectra(plane, 16384, stack=n //
      16384)``: as many samples per output spectrum, in incoherent stacks of 16384-point transforms.

The `_t256` and `_t512` rows repeat a row under a smaller workgroup (BBT_LSPEC_THREADS; the default is 1024),
without the yardsticks.

`bytes_model` is 14 bytes per input value (4 read, 4 + 4 through the scratch, 2 written) and
`fraction_of_copy_rate` that traffic's rate over the copy's (which moves 8 bytes per value)."""
import os
import sys

import bench_rows
from bench_rows import events_ms, reread

sys.path.insert(0, bench_rows.ROOT)

ROWS = {
    'n20': dict(length=1 << 20, ndm=512, n=1 << 20, stack=1),
    'n22': dict(length=1 << 22, ndm=256, n=1 << 22, stack=1),
    'n15_stack32': dict(length=1 << 20, ndm=512, n=1 << 15, stack=32),
    # the same under other workgroup sizes (BBT_LSPEC_THREADS), without the yardsticks
    'n20_t256': dict(length=1 << 20, ndm=512, n=1 << 20, stack=1, threads=256),
    'n20_t512': dict(length=1 << 20, ndm=512, n=1 << 20, stack=1, threads=512),
    'n22_t256': dict(length=1 << 22, ndm=256, n=1 << 22, stack=1, threads=256),
    'n22_t512': dict(length=1 << 22, ndm=256, n=1 << 22, stack=1, threads=512),
    'n15_stack32_t256': dict(length=1 << 20, ndm=512, n=1 << 15, stack=32, threads=256),
    'n15_stack32_t512': dict(length=1 << 20, ndm=512, n=1 << 15, stack=32, threads=512),
}
ROW_LIMIT = 400          # seconds a row may take
RATE = 1e3
SHORT = 16384


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip
    row = ROWS[name]
    length, ndm, n, stack = row['length'], row['ndm'], row['n'], row['stack']
    if 'threads' in row:
        os.environ['BBT_LSPEC_THREADS'] = str(row['threads'])
    bt.hip.set_device(0)
    rng = np.random.default_rng(7)
    x = np.tile(rng.standard_normal((1 << 16, ndm), dtype=np.float32), (length >> 16, 1))
    t0 = bt.Time('2020-01-01T00:00:00')
    plane = bt.DeviceStream(x, t0, RATE, samples_per_frame=SHORT, frequency=600e6, sideband=1)
    del x
    values = length * ndm
    line = dict(row=name, device=hip.device_name(), length=length, ndm=ndm, n=n, stack=stack, reps=reps,
                plane_bytes=values * 4, bytes_model=values * 14)

    def timed(task):
        times = events_ms(lambda: reread(task), 2, reps)
        return round(min(times), 3), round(float(np.median(times)), 3)

    sp = bt.LongSpectra(plane, n, stack)
    plan = hip.LongSpectraPlan(n, stack, ndm)
    line.update(plan.info(sp.spectra_budget))
    plan.close()
    line['launches'] = 2 * stack * -(-((ndm + 1) // 2) // line['pairs_per_launch'])
    line['long_ms_min'], line['long_ms_med'] = timed(sp)
    sp.close()
    if 'threads' in row:
        return line
    src, dst = hip.DeviceArray((values,), np.float32), hip.DeviceArray((values,), np.float32)
    hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))
    c = events_ms(lambda: dst.copy_from_device(src), 2, reps)
    del src, dst
    line.update(copy_ms=round(min(c), 3), copy_ms_med=round(float(np.median(c)), 3))
    line['long_over_copy'] = round(line['long_ms_min'] / line['copy_ms'], 2)
    line['long_tb_per_s'] = round(line['bytes_model'] / line['long_ms_min'] / 1e9, 3)
    line['copy_tb_per_s'] = round(values * 8 / line['copy_ms'] / 1e9, 3)
    line['fraction_of_copy_rate'] = round(line['long_tb_per_s'] / line['copy_tb_per_s'], 3)
    short = bt.periodicity.fluctuation_spectra(plane, SHORT, stack=n * stack // SHORT)
    assert short.shape[0] == length // (n * stack)
    line['short_ms_min'], line['short_ms_med'] = timed(short)
    line['long_over_short'] = round(line['long_ms_min'] / line['short_ms_min'], 2)
    return line


if __name__ == '__main__':
    sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'lspec_bench.jsonl'))
