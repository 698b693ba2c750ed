"""`Standardize` and `BoxcarSearch` on a resident (time, DM) plane against two yardsticks from the same
run, one JSON line per row (dev tool; needs a GPU).

    python tools/bench_sps.py [--out FILE] [--reps N] [row ...]

Rows: float32 noise planes of (2^16, 512) and (2^18, 512), resident in HBM.  Per plane `Standardize`
with blocks of 4096 and `BoxcarSearch` with blocks of 256 start times and 1, 6, 10 and 13 widths,
each on the plane itself.  Every row runs in a child process of its own under a time limit, and the
first row that fails ends the run.

Timed with device events around ``read_device()`` of the whole result (the cache dropped before
every repeat): 2 warm-up reads, then ``--reps`` timed ones; the minimum and the median are reported.

  `copy_ms`: a device-to-device copy of the plane's bytes.
  `dmt_ms`: `DMTrials` making a plane of 512 trials from a (2^16, 1024) stream whose sweep spans about
      4000 samples (the 512-trial row of tools/bench_dmtrials.py); on the 2^16 row only.

`k13_over_copy` and `k13_over_dmt` are the 13-width search over those.  The `fuse_*`, `width_*` and
`split_*` rows repeat the 13-width search of the 2^16 plane under other tilings (BBT_SPS_FUSE levels
per pass, BBT_SPS_WIDTH elements per workgroup, BBT_SPS_SPLIT threads per block and element), and the
`rows_*` rows `Standardize` under BBT_SPS_STD_ROWS."""
import os
import sys

import bench_rows
from bench_rows import events_ms, reread

sys.path.insert(0, bench_rows.ROOT)

ROWS = {
    'n16_d512': dict(n=1 << 16, ndm=512, dmt=True),
    'n18_d512': dict(n=1 << 18, ndm=512),
    'fuse_1': dict(n=1 << 16, ndm=512, env=dict(BBT_SPS_FUSE=1), widths=(13,), yardsticks=False),
    'fuse_3': dict(n=1 << 16, ndm=512, env=dict(BBT_SPS_FUSE=3), widths=(13,), yardsticks=False),
    'width_16': dict(n=1 << 16, ndm=512, env=dict(BBT_SPS_WIDTH=16), widths=(13,), yardsticks=False),
    'width_32': dict(n=1 << 16, ndm=512, env=dict(BBT_SPS_WIDTH=32), widths=(13,), yardsticks=False),
    'split_1': dict(n=1 << 16, ndm=512, env=dict(BBT_SPS_SPLIT=1), widths=(13,), yardsticks=False),
    'rows_1': dict(n=1 << 16, ndm=512, env=dict(BBT_SPS_STD_ROWS=1), widths=(), yardsticks=False),
    'rows_16': dict(n=1 << 16, ndm=512, env=dict(BBT_SPS_STD_ROWS=16), widths=(), yardsticks=False),
}
ROW_LIMIT = 300          # seconds a row may take
RATE = 1e4
BLOCK, STD_BLOCK = 256, 4096
WIDTHS = (1, 6, 10, 13)
SPAN = 4000


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip, search
    row = ROWS[name]
    n, ndm = row['n'], row['ndm']
    for key, value in row.get('env', {}).items():
        os.environ[key] = str(value)
    bt.hip.set_device(0)
    rng = np.random.default_rng(7)
    x = rng.standard_normal((n, ndm), dtype=np.float32)
    t0 = bt.Time('2020-01-01T00:00:00')
    plane = bt.DeviceStream(x, t0, RATE, samples_per_frame=n)
    info = hip.sps_info()
    line = dict(row=name, device=hip.device_name(), n=n, ndm=ndm, block=BLOCK, std_block=STD_BLOCK, reps=reps,
                plane_bytes=n * ndm * 4, width=info['width'], fuse=info['fuse'], split=info['split'],
                std_rows=info['std_rows'])

    def timed(task):
        times = events_ms(lambda: reread(task), 2, reps)
        return round(min(times), 3), round(float(np.median(times)), 3)

    st = bt.Standardize(plane, STD_BLOCK, samples_per_frame=n)
    line['std_ms_min'], line['std_ms_med'] = timed(st)
    st.close()
    for k in row.get('widths', WIDTHS):
        bs = bt.BoxcarSearch(plane, BLOCK, k, samples_per_frame=n // BLOCK)
        line[f'k{k}_ms_min'], line[f'k{k}_ms_med'] = timed(bs)
        line[f'k{k}_launches'] = -(-bs.shape[0] // bs._chunk_size())
        line[f'k{k}_scratch_bytes'] = bs._plan.info()['scratch_bytes']
        bs.close()
    if row.get('yardsticks', True):
        words = n * ndm
        src, dst = hip.DeviceArray((words,), np.float32), hip.DeviceArray((words,), np.float32)
        hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))
        c = events_ms(lambda: dst.copy_from_device(src), 2, reps)
        line.update(copy_ms=round(min(c), 3), copy_ms_med=round(float(np.median(c)), 3))
        line['std_over_copy'] = round(line['std_ms_min'] / line['copy_ms'], 2)
        for k in WIDTHS:
            line[f'k{k}_over_copy'] = round(line[f'k{k}_ms_min'] / line['copy_ms'], 2)
        del src, dst
    if row.get('dmt'):
        nchan = 1024
        y = rng.random((n, nchan), dtype=np.float32)
        dh = bt.DeviceStream(y, t0, RATE, samples_per_frame=n, frequency=np.linspace(400.3e6, 799.1e6, nchan), sideband=1)
        unit = search.dm_trial_shifts(dh, [1.])
        dt = bt.DMTrials(dh, np.linspace(0., SPAN / float(np.ptp(unit)), ndm), samples_per_frame=n)
        line['dmt_ms'], line['dmt_ms_med'] = timed(dt)
        line['dmt_n_out'] = dt.shape[0]
        dt.close()
        line['std_over_dmt'] = round(line['std_ms_min'] / line['dmt_ms'], 3)
        for k in WIDTHS:
            line[f'k{k}_over_dmt'] = round(line[f'k{k}_ms_min'] / line['dmt_ms'], 3)
    return line


if __name__ == '__main__':
    sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'sps_bench.jsonl'))
