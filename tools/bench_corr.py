"""`Correlate` on resident streams beside a device-to-device copy of the input's bytes and, for two inputs,
beside `Integrate(Power(...))`, all from the same run: one JSON line per row (dev tool; needs a GPU).

    python tools/bench_corr.py [--out FILE] [--reps N] [row ...]

Rows: `a16`: a complex64 noise stream of (2^14, 1024, 16) resident in HBM, correlated in blocks of 1024;
`a64`: (2^12, 1024, 64) in blocks of 1024; `long16`: (2^22, 16) in blocks of 2^20, one element and a long
integration; `a2`: (2^16, 1024, 2) in blocks of 1024, also under `Integrate(Power(...), 1024)`.  Every row
runs in a child process of its own under a time limit, and the first row that fails ends the run.

Timed with device events around ``read_device()`` of the whole result (the cache dropped before every
read).  The candidates of a row TAKE TURNS -- the copy, `Correlate`, and `Integrate(Power)` where there is
one -- two warm-up turns, then ``--reps`` timed ones; the minimum of each is reported, with its ratio to the
copy (`*_over_copy`), the input bytes per second and the real multiply-adds per second of the Gram
matrix's upper triangle as the rule counts them (4 per baseline and sample, `useful_tflops` at 2 flops
each).  `pack`, `tiles` and `waves` say how a wave was cut."""
import os
import sys

import bench_rows
from bench_rows import reread, take_turns

sys.path.insert(0, bench_rows.ROOT)

ROWS = {
    'a16': dict(shape=(1 << 14, 1024, 16), n=1024),
    'a64': dict(shape=(1 << 12, 1024, 64), n=1024),
    'long16': dict(shape=(1 << 22, 16), n=1 << 20),
    'a2': dict(shape=(1 << 16, 1024, 2), n=1024),
}
ROW_LIMIT = 300          # seconds a row may take
RATE = 1e4
WARM = 2


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip
    row = ROWS[name]
    shape, n = row['shape'], row['n']
    for knob in ('BBT_CORR_PACK', 'BBT_CORR_WAVES'):
        os.environ.pop(knob, None)
    bt.hip.set_device(0)
    rng = np.random.default_rng(7)
    t0 = bt.Time('2020-01-01T00:00:00')
    # the stream is made in HBM from one chunk of noise, repeated: the values do not matter to the clock
    per = int(np.prod(shape[1:]))
    rows = max(1, min(shape[0], (1 << 23) // per))
    chunk = (rng.standard_normal((rows,) + shape[1:], dtype=np.float32)
             + 1j * rng.standard_normal((rows,) + shape[1:], dtype=np.float32)).astype(np.complex64)
    data = hip.DeviceArray(shape, np.complex64)
    for start in range(0, shape[0], rows):
        data[start:start + rows].copy_from_host(chunk[:min(rows, shape[0] - start)])
    del chunk
    a = shape[-1]
    meta = dict(polarization=np.array(['X', 'Y'])) if a == 2 else {}
    ih = bt.DeviceStream(data, t0, RATE, samples_per_frame=shape[0], **meta)
    blocks = shape[0] // n
    corr = bt.Correlate(ih, n, samples_per_frame=blocks)
    piece = min(corr._piece_size(), shape[0])
    info = hip.corr_info(a, per // a, n, 0, piece)
    nbytes = int(np.prod(shape)) * 8
    src, dst = hip.DeviceArray((nbytes,), np.uint8), hip.DeviceArray((nbytes,), np.uint8)
    hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))
    candidates = {'copy': lambda: dst.copy_from_device(src), 'corr': lambda: reread(corr)}
    if a == 2:
        power = bt.Integrate(bt.Power(ih), n, samples_per_frame=blocks)
        candidates['power'] = lambda: reread(power)
    times = take_turns(candidates, WARM, reps)
    line = dict(row=name, device=hip.device_name(), shape=list(shape), n=n, reps=reps, bytes=nbytes, piece=piece,
                pack=info['pack'], tiles=info['tiles'], waves=info['waves'], lds_bytes=info['lds_bytes'],
                scratch_bytes=info['scratch_bytes'])
    for key, values in times.items():
        line[f'{key}_ms'] = round(min(values), 3)
        line[f'{key}_ms_med'] = round(float(np.median(values)), 3)
    for key in candidates:
        if key != 'copy':
            line[f'{key}_over_copy'] = round(line[f'{key}_ms'] / line['copy_ms'], 2)
    line['corr_gbytes_per_s'] = round(nbytes / line['corr_ms'] / 1e6, 1)
    line['useful_tflops'] = round(8 * (a * (a + 1) // 2) * (per // a) * blocks * n / line['corr_ms'] / 1e9, 2)
    if a == 2:
        line['corr_over_power'] = round(line['corr_ms'] / line['power_ms'], 2)
    return line


if __name__ == '__main__':
    sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'corr_bench.jsonl'))
