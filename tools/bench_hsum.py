"""`Whiten` and `HarmonicSearch` on a resident stack of fluctuation spectra against two yardsticks from
the same run, one JSON line per row (dev tool; needs a GPU).

    python tools/bench_hsum.py [--out FILE] [--reps N] [row ...]

Rows: a float32 stack of (64, 8193, 512) -- 64 spectra of 16384-point transforms of 512 trials --
of exponential noise, resident in HBM.  `Whiten` with blocks of 128 bins and `HarmonicSearch` with
blocks of 64 bins and 1, 3, 5 and 6 levels, each on the stack itself.  Every row runs in a child
process of its own under a time limit, and the first row that fails ends the run.

Timed with device events around ``read_device()`` of the whole result (the cache dropped before
every repeat): 2 warm-up reads, then ``--reps`` timed ones; the minimum and the median are reported.

  `copy_ms`: a device-to-device copy of the stack's bytes.
  `spectra_ms`: `fluctuation_spectra(plane, 16384)` making a stack of that shape from a resident (2^20,
      512) float32 plane (one transform per spectrum: ``stack=1``, so that the plane is 2 GiB, not 16).

`k5_over_copy` and `k5_over_spectra` are the 5-level search over those.  The `width_*` and `split_*`
rows repeat the 5-level search under other tilings (BBT_HSUM_WIDTH elements per workgroup,
BBT_HSUM_SPLIT threads per spectrum, block and element), and the `rows_*` rows `Whiten` under
BBT_HSUM_ROWS."""
import os
import sys

import bench_rows
from bench_rows import events_ms, reread

sys.path.insert(0, bench_rows.ROOT)

ROWS = {
    'stack': dict(spectra=True),
    'width_16': dict(env=dict(BBT_HSUM_WIDTH=16), levels=(5,), yardsticks=False),
    'width_16_split_4': dict(env=dict(BBT_HSUM_WIDTH=16, BBT_HSUM_SPLIT=4), levels=(5,), yardsticks=False),
    'width_32': dict(env=dict(BBT_HSUM_WIDTH=32), levels=(5,), yardsticks=False),
    'split_1': dict(env=dict(BBT_HSUM_SPLIT=1), levels=(5,), yardsticks=False),
    'split_2': dict(env=dict(BBT_HSUM_SPLIT=2), levels=(5,), yardsticks=False),
    'rows_1': dict(env=dict(BBT_HSUM_ROWS=1), levels=(), yardsticks=False),
    'rows_16': dict(env=dict(BBT_HSUM_ROWS=16), levels=(), yardsticks=False),
}
ROW_LIMIT = 300          # seconds a row may take
RATE = 1e4
N_SPEC, N_FFT, NDM = 64, 16384, 512
NBIN = N_FFT // 2 + 1
BLOCK, WHITEN_BLOCK = 64, 128
LEVELS = (1, 3, 5, 6)


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip
    row = ROWS[name]
    for key, value in row.get('env', {}).items():
        os.environ[key] = str(value)
    bt.hip.set_device(0)
    rng = np.random.default_rng(7)
    x = rng.standard_exponential((N_SPEC, NBIN, NDM), dtype=np.float32)
    t0 = bt.Time('2020-01-01T00:00:00')
    stack = bt.DeviceStream(x, t0, RATE / N_FFT, samples_per_frame=N_SPEC)
    del x
    info = hip.hsum_info()
    line = dict(row=name, device=hip.device_name(), n_spec=N_SPEC, nbin=NBIN, ndm=NDM, block=BLOCK,
                whiten_block=WHITEN_BLOCK, reps=reps, stack_bytes=N_SPEC * NBIN * NDM * 4, width=info['width'],
                split=info['split'], rows=info['rows'])

    def timed(task):
        times = events_ms(lambda: reread(task), 2, reps)
        return round(min(times), 3), round(float(np.median(times)), 3)

    wh = bt.Whiten(stack, WHITEN_BLOCK)
    line['whiten_ms_min'], line['whiten_ms_med'] = timed(wh)
    line['whiten_launches'] = -(-N_SPEC // wh._chunk_size())
    wh.close()
    for k in row.get('levels', LEVELS):
        hs = bt.HarmonicSearch(stack, BLOCK, k)
        line[f'k{k}_ms_min'], line[f'k{k}_ms_med'] = timed(hs)
        line[f'k{k}_launches'] = -(-N_SPEC // hs._chunk_size())
        hs.close()
    if row.get('yardsticks', True):
        words = N_SPEC * NBIN * NDM
        src, dst = hip.DeviceArray((words,), np.float32), hip.DeviceArray((words,), np.float32)
        hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))
        c = events_ms(lambda: dst.copy_from_device(src), 2, reps)
        line.update(copy_ms=round(min(c), 3), copy_ms_med=round(float(np.median(c)), 3))
        line['whiten_over_copy'] = round(line['whiten_ms_min'] / line['copy_ms'], 2)
        for k in LEVELS:
            line[f'k{k}_over_copy'] = round(line[f'k{k}_ms_min'] / line['copy_ms'], 2)
        del src, dst
    if row.get('spectra'):
        stack.close()
        del stack
        y = rng.standard_normal((N_SPEC * N_FFT, NDM), dtype=np.float32)
        plane = bt.DeviceStream(y, t0, RATE, samples_per_frame=N_FFT, frequency=600e6, sideband=1)
        del y
        sp = bt.periodicity.fluctuation_spectra(plane, N_FFT)
        assert sp.shape == (N_SPEC, NBIN, NDM)
        line['spectra_ms'], line['spectra_ms_med'] = timed(sp)
        line['plane_bytes'] = N_SPEC * N_FFT * NDM * 4
        line['whiten_over_spectra'] = round(line['whiten_ms_min'] / line['spectra_ms'], 3)
        for k in LEVELS:
            line[f'k{k}_over_spectra'] = round(line[f'k{k}_ms_min'] / line['spectra_ms'], 3)
    return line


if __name__ == '__main__':
    sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'hsum_bench.jsonl'))
