"""`DMTrials` on a resident stream against two yardsticks from the same run, one JSON line per row
(dev tool; needs a GPU).

    python tools/bench_dmtrials.py [--out FILE] [--reps N] [row ...]

Rows: a (2^16, 1024) float32 stream with 128, 512 and 2048 trials, and a (2^18, 256) one with 512
trials; channels spread linearly over 400.3 ... 799.1 MHz at 10 kHz, trials from 0 to the DM whose
sweep spans about 4000 samples.  Every row runs in a child process of its own under a time limit,
and the first row that fails ends the run.

Timed with device events around ``read_device()`` of the whole trial plane (the cache dropped before
every repeat): 2 warm-up reads, then ``--reps`` timed ones; the minimum and the median are reported.
``adds_per_s`` counts n_out * ndm * nchan float adds over the minimum.

  (a) `a_ms`: what the package could do before `DMTrials` -- one `DedisperseSamples` pass per trial.
      Timed on 16 trials spread over the grid and scaled by ndm / 16.  The channel sum that route
      also needs is NOT in it (the package had no kernel for it), so (a) is a lower bound.
  (b) `b_ms`: a device-to-device copy of as many bytes as the input plus the output.

The `tile_*` rows repeat the 512-trial row under other tilings (BBT_DMT_TILE output times per
workgroup, BBT_DMT_TRIALS trials per thread)."""
import os
import sys

import bench_rows
from bench_rows import events_ms, reread

sys.path.insert(0, bench_rows.ROOT)

ROWS = {
    'n16_c1024_d128': dict(n=1 << 16, nchan=1024, ndm=128),
    'n16_c1024_d512': dict(n=1 << 16, nchan=1024, ndm=512),
    'n16_c1024_d2048': dict(n=1 << 16, nchan=1024, ndm=2048),
    'n18_c256_d512': dict(n=1 << 18, nchan=256, ndm=512),
    'tile_256_1': dict(n=1 << 16, nchan=1024, ndm=512, tile=256, trials=1, yardsticks=False),
    'tile_256_4': dict(n=1 << 16, nchan=1024, ndm=512, tile=256, trials=4, yardsticks=False),
    'tile_256_16': dict(n=1 << 16, nchan=1024, ndm=512, tile=256, trials=16, yardsticks=False),
    'tile_64_8': dict(n=1 << 16, nchan=1024, ndm=512, tile=64, trials=8, yardsticks=False),
}
ROW_LIMIT = 300          # seconds a row may take
RATE = 1e4
SPAN = 4000


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip, search
    row = ROWS[name]
    n, nchan, ndm = row['n'], row['nchan'], row['ndm']
    if 'tile' in row:
        os.environ['BBT_DMT_TILE'], os.environ['BBT_DMT_TRIALS'] = str(row['tile']), str(row['trials'])
    bt.hip.set_device(0)
    rng = np.random.default_rng(7)
    x = rng.random((n, nchan), dtype=np.float32)
    freq = np.linspace(400.3e6, 799.1e6, nchan)
    dh = bt.DeviceStream(x, bt.Time('2020-01-01T00:00:00'), RATE, samples_per_frame=n, frequency=freq, sideband=1)
    unit = search.dm_trial_shifts(dh, [1.])
    dm_max = SPAN / float(np.ptp(unit))
    dms = np.linspace(0., dm_max, ndm)
    dt = bt.DMTrials(dh, dms, samples_per_frame=n)
    span, n_out = int(np.ptp(dt.shifts)), dt.shape[0]

    times = events_ms(lambda: reread(dt), 2, reps)
    info = dt._plan.info()
    adds = n_out * ndm * nchan
    line = dict(row=name, device=hip.device_name(), n=n, nchan=nchan, ndm=ndm, span=span, n_out=n_out,
                tile=info['tile'], trials=info['trials'], reps=reps, ms_min=round(min(times), 3),
                ms_med=round(float(np.median(times)), 3), adds_per_s=round(adds / (min(times) * 1e-3), 0),
                in_bytes=n * nchan * 4, out_bytes=n_out * ndm * 4)
    if row.get('yardsticks', True):
        # (a) one DedisperseSamples pass per trial, 16 of the trials, no channel sum
        picked = dms[np.linspace(0, ndm - 1, 16).astype(int)]
        tasks = [bt.DedisperseSamples(dh, dm, samples_per_frame=n - span) for dm in picked]

        def per_trial():
            for t in tasks:
                t.invalidate_cache()
                t.seek(0)
                t.read_device(n_out)

        a = events_ms(per_trial, 1, 3)
        line.update(a_ms_16_trials=round(min(a), 3), a_ms=round(min(a) * ndm / 16., 3),
                    a_note='16 DedisperseSamples passes scaled by ndm / 16; the channel sum is not included')
        for t in tasks:
            t.close()
        # (b) a copy of input + output bytes
        words = (line['in_bytes'] + line['out_bytes']) // 4
        src, dst = hip.DeviceArray((words,), np.float32), hip.DeviceArray((words,), np.float32)
        hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))
        b = events_ms(lambda: dst.copy_from_device(src), 2, 5)
        line.update(b_ms=round(min(b), 3), speedup_over_a=round(line['a_ms'] / line['ms_min'], 2),
                    b_over_time=round(min(b) / line['ms_min'], 4))
    return line


if __name__ == '__main__':
    sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'dmtrials_bench.jsonl'))
