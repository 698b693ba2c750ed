"""Generate tests/golden/conversion_vectors.npz from the REAL reference's `Real2Complex`.

Run from this directory with a checkout of the reference (mhvk/baseband-tasks)
on the Python path and astropy installed, as for make_fold_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python3 -W ignore make_conversion_golden.py

(the committed vectors: CPython 3.9, numpy 1.26, astropy 4.3.1).

Only data are written.  Per case: the input stream (seeded small integers, kept
as int8 to stay small; the stream itself is float32), the reference's complex64
output and, as JSON, the output frame length, the frame count, the input's
samples_per_frame, frequency and sideband, and the output's shape, sample rate,
frequency, sideband, samples_per_frame and dtype.  The reference works on 1-d
streams only, so every input is 1-d.
"""
import json
import os

import numpy as np

for _name, _fn in (('asscalar', lambda a: np.asarray(a).item()),
                   ('alen', lambda a: len(np.asarray(a)))):
    if not hasattr(np, _name):
        setattr(np, _name, _fn)

from astropy import units as u            # noqa: E402
from astropy.time import Time             # noqa: E402

from baseband_tasks.generators import StreamGenerator                 # noqa: E402
from baseband_tasks.conversion import Real2Complex                    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
T0 = '2010-11-12T13:14:15'
RATE = 64000.                            # Hz

# (output frame length M, frames, extra input samples past the last whole frame, options)
#   default: Real2Complex(ih) with ih.samples_per_frame = 2 M;  else samples_per_frame = M given
#   and ih.samples_per_frame = M (the reference reads its input frame by frame either way)
CASES = [
    dict(M=2, frames=3, extra=1),
    dict(M=3, frames=3, extra=0),
    dict(M=7, frames=3, extra=5),
    dict(M=500, frames=3, extra=0, frequency=300e6, sideband=-1),
    dict(M=1000, frames=2, extra=37, default=True, frequency=1400e6, sideband=1),
    dict(M=1024, frames=2, extra=0),
    dict(M=1215, frames=2, extra=0),
    dict(M=4096, frames=2, extra=0),
    dict(M=6174, frames=2, extra=0),
    dict(M=10000, frames=2, extra=0),
    dict(M=16384, frames=2, extra=0),
]


def reference_stream(data, spf, frequency=None, sideband=None):
    def frame(sh):
        return data[sh.tell():sh.tell() + sh.samples_per_frame]
    kw = {}
    if frequency is not None:
        kw = dict(frequency=frequency * u.Hz, sideband=sideband)
    return StreamGenerator(frame, shape=data.shape, start_time=Time(T0, precision=9),
                           sample_rate=RATE * u.Hz, samples_per_frame=spf, dtype=data.dtype, **kw)


def main():
    rng = np.random.default_rng(20261017)
    out = {}
    for i, case in enumerate(CASES):
        m, frames = case['M'], case['frames']
        n = 2 * m * frames + case['extra']
        raw = rng.integers(-20, 21, size=n).astype(np.int8)
        data = raw.astype(np.float32)
        spf_in = 2 * m if case.get('default') else m
        ih = reference_stream(data, spf_in, case.get('frequency'), case.get('sideband'))
        task = Real2Complex(ih) if case.get('default') else Real2Complex(ih, samples_per_frame=m)
        result = task.read()
        assert result.shape == (m * frames,) and result.dtype == np.complex64, (i, result.shape, result.dtype)
        freq = getattr(task, 'frequency', None)
        meta = dict(case, ih_samples_per_frame=spf_in, shape=list(task.shape),
                    sample_rate=float(task.sample_rate.to_value(u.Hz)),
                    samples_per_frame=int(task.samples_per_frame), dtype=str(task.dtype),
                    out_frequency=None if freq is None else float(freq.to_value(u.Hz)),
                    out_sideband=None if freq is None else int(task.sideband),
                    start_time=task.start_time.isot, repr=repr(task).split('\n')[0])
        key = f'case{i:02d}'
        out[f'{key}/meta'] = np.array(json.dumps(meta))
        out[f'{key}/input'] = raw
        out[f'{key}/output'] = result
    np.savez_compressed(os.path.join(HERE, 'conversion_vectors.npz'), **out)
    print('wrote', len(CASES), 'cases')


if __name__ == '__main__':
    main()
