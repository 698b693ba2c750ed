"""Generate tests/golden/shaping_vectors.npz from the REAL reference's shaping and combining tasks.

Run from this directory with a checkout of the reference (mhvk/baseband-tasks)
on the Python path and astropy installed, as for make_conversion_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python3 -W ignore make_shaping_golden.py

(the committed vectors: CPython 3.9, numpy 1.26, astropy 4.3.1).

Only data are written.  Per case: the input stream(s) (seeded small integers,
kept as int8; the streams themselves are float32), the reference's output (int8
too: moving samples does not change them) and, as JSON, the case description,
the output's shape, start time, samples_per_frame and its frequency, sideband
and polarization (None where the reference has none).

With that interpreter the reference's `Stack` raises ``TypeError: concatenate()
got an unexpected keyword argument 'dtype'`` as soon as ``frequency`` is an astropy
`Quantity` (np.stack on Quantities: a mismatch of those two versions), so the
`Stack` and `CombineStreams` cases give their streams unit-less frequencies, in
Hz; the other cases use `Quantity`.  Frequencies are compared by value.
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
from baseband_tasks import shaping, combining                       # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
T0 = '2010-11-12T13:14:15'
RATE = 1000.                             # Hz
N = 240                                  # samples per stream
SPF = 40


def freqs(n):
    return 300e6 + 1e6 * np.arange(n)


# Streams: sample shape, frequency / sideband / polarization (broadcastable), start offset in samples.
# Cases: (class, streams, positional arguments, keyword arguments); items are written so that JSON
# can hold them: ['slice', a, b, c] is slice(a, b, c), a list is a list index, ['tuple', ...] a tuple.
S8 = dict(shape=(8,), frequency=np.repeat(freqs(4), 2), sideband=1, polarization=np.tile(['L', 'R'], 4))
S42 = dict(shape=(4, 2), frequency=freqs(4)[:, None], sideband=np.array([1, -1]), polarization=np.array(['X', 'Y']))
S4 = dict(shape=(4,), frequency=freqs(4), sideband=-1, polarization='X')
S4B = dict(shape=(4,), frequency=freqs(4) + 16e6, sideband=-1, polarization='Y', first=7)
S1X = dict(shape=(), frequency=300e6, sideband=1, polarization='X')
S1Y = dict(shape=(), frequency=300e6, sideband=1, polarization='Y', first=3)
S32 = dict(shape=(3, 2), frequency=freqs(3)[:, None], sideband=1, polarization=np.array(['X', 'Y']))
S32B = dict(shape=(3, 2), frequency=freqs(3)[:, None] + 8e6, sideband=1, polarization=np.array(['X', 'Y']), first=11)
S = ['slice']

CASES = [
    ('Reshape', [S8], [[4, 2]], {}),
    ('Transpose', [S42], [[2, 1]], {}),
    ('ReshapeAndTranspose', [S8], [[4, 2], [2, 1]], {}),
    ('GetItem', [S42], [1], {}),
    ('GetItem', [S42], [S + [1, 3, None]], {}),
    ('GetItem', [S8], [S + [None, None, -3]], {}),
    ('GetItem', [S8], [[5, 0, 0, 2]], {}),
    ('GetItem', [S42], [['tuple', S + [None, None, 2], 1]], {}),
    ('GetItem', [S42], [['tuple', [3, 1], S + [None, None, -1]]], {}),
    ('GetSlice', [S42], [S + [10, -10, None]], {}),
    ('GetSlice', [S42], [['tuple', S + [35, 175, None], S + [1, None, None], 0]], {}),
    ('ChangeSampleShape', [S42], ['swapaxes'], {}),
    ('Concatenate', [S4, S4B], [], dict(axis=1)),
    ('Concatenate', [S32, S32B], [], dict(axis=-1)),
    ('Concatenate', [S32, S32B], [], dict(axis=1, samples_per_frame=25)),
    ('Stack', [S4, S4B], [], dict(axis=1, unitless=True)),
    ('Stack', [S4, S4B], [], dict(axis=2, unitless=True)),
    ('Stack', [S1X, S1Y], [], dict(axis=-1, unitless=True)),
    ('Stack', [S32, S32B, S32], [], dict(axis=2, samples_per_frame=32, unitless=True)),
    ('CombineStreams', [S1X, S1Y], ['stack'], dict(unitless=True)),
]

CALLABLES = {'swapaxes': lambda data: data.swapaxes(1, 2),
             'stack': lambda data: np.stack(data, axis=1)}


def decode(arg):
    if isinstance(arg, list) and arg and arg[0] == 'slice':
        return slice(*arg[1:])
    if isinstance(arg, list) and arg and arg[0] == 'tuple':
        return tuple(decode(a) for a in arg[1:])
    if isinstance(arg, str):
        return CALLABLES[arg]
    return arg


def reference_stream(data, spec, unitless):
    def frame(sh):
        return data[sh.tell():sh.tell() + sh.samples_per_frame]
    frequency = np.asarray(spec['frequency'], dtype=float)
    start = Time(T0, precision=9) + spec.get('first', 0) / RATE * u.s
    return StreamGenerator(frame, shape=data.shape, start_time=start, sample_rate=RATE * u.Hz,
                           samples_per_frame=SPF, dtype=data.dtype,
                           frequency=frequency if unitless else frequency * u.Hz,
                           sideband=spec['sideband'], polarization=spec['polarization'])


def plain(value):
    if value is None:
        return None
    if hasattr(value, 'to_value'):
        value = value.to_value(u.Hz)
    value = np.asarray(value)
    return dict(shape=list(value.shape), values=value.ravel().tolist())


def main():
    rng = np.random.default_rng(20261018)
    out = {}
    for i, (name, specs, args, kwargs) in enumerate(CASES):
        kwargs = dict(kwargs)
        unitless = kwargs.pop('unitless', False)
        raws = [rng.integers(-100, 101, size=(N,) + tuple(s['shape'])).astype(np.int8) for s in specs]
        streams = [reference_stream(r.astype(np.float32), s, unitless) for r, s in zip(raws, specs)]
        cls = getattr(shaping, name, None) or getattr(combining, name)
        is_shaping = hasattr(shaping, name)
        if name in ('Reshape', 'ReshapeAndTranspose', 'Transpose'):
            task = cls(streams[0], *[tuple(a) for a in args])        # (shapes and axes: tuples)
        else:
            task = cls(streams[0] if is_shaping else streams, *[decode(a) for a in args], **kwargs)
        result = task.read()
        assert result.dtype == np.float32 and np.all(result == np.round(result))
        meta = dict(cls=name, args=args, kwargs=kwargs, unitless=unitless,
                    streams=[dict(shape=list(s['shape']), first=s.get('first', 0),
                                  frequency=plain(np.asarray(s['frequency'], dtype=float)),
                                  sideband=plain(s['sideband']), polarization=plain(s['polarization']))
                             for s in specs],
                    rate=RATE, t0=T0, samples_per_frame_in=SPF,
                    shape=list(task.shape), start_time=task.start_time.isot,
                    samples_per_frame=int(task.samples_per_frame),
                    frequency=plain(getattr(task, 'frequency', None)),
                    sideband=plain(getattr(task, 'sideband', None)),
                    polarization=plain(getattr(task, 'polarization', None)))
        key = f'case{i:02d}'
        out[f'{key}/meta'] = np.array(json.dumps(meta))
        for k, r in enumerate(raws):
            out[f'{key}/input{k}'] = r
        out[f'{key}/output'] = result.astype(np.int8)
    np.savez_compressed(os.path.join(HERE, 'shaping_vectors.npz'), **out)
    print('wrote', len(CASES), 'cases')


if __name__ == '__main__':
    main()
