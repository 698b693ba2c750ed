"""Helpers shared by test_shaping_host.py and test_shaping_gpu.py: the golden cases of
tests/golden/shaping_vectors.npz (made by the real reference: make_shaping_golden.py) rebuilt
with this package's classes."""
import json
import os

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import units as u

HERE = os.path.dirname(os.path.abspath(__file__))

CALLABLES = {'swapaxes': lambda data: data.swapaxes(1, 2),
             'stack': lambda data: np.stack(data, axis=1)}
SHAPING = ('Reshape', 'Transpose', 'ReshapeAndTranspose', 'GetItem', 'GetSlice', 'ChangeSampleShape')


def load():
    z = np.load(os.path.join(HERE, 'golden', 'shaping_vectors.npz'))
    keys = sorted({k.split('/')[0] for k in z.files})
    cases = []
    for key in keys:
        meta = json.loads(str(z[f'{key}/meta']))
        inputs = [z[f'{key}/input{k}'] for k in range(len(meta['streams']))]
        cases.append((key, meta, inputs, z[f'{key}/output']))
    return cases


def decode(arg):
    if isinstance(arg, list) and arg and arg[0] == 'slice':
        return slice(*arg[1:])
    if isinstance(arg, list) and arg and arg[0] == 'tuple':
        return tuple(decode(a) for a in arg[1:])
    if isinstance(arg, str):
        return CALLABLES[arg]
    return arg


def unplain(value, dtype=None):
    if value is None:
        return None
    return np.array(value['values'], dtype=dtype).reshape(value['shape'])


def host_stream(meta, k, data):
    """Stream k of a case as a host `StreamGenerator` of float32 (what the reference was given)."""
    spec = meta['streams'][k]
    data = np.ascontiguousarray(data, dtype=np.float32)

    def frame(sh):
        return data[sh.tell():sh.tell() + sh.samples_per_frame]
    start = u.Time(meta['t0']) + spec['first'] / meta['rate']
    return bt.StreamGenerator(frame, shape=data.shape, start_time=start, sample_rate=meta['rate'],
                              samples_per_frame=meta['samples_per_frame_in'], dtype=np.float32,
                              frequency=unplain(spec['frequency']), sideband=unplain(spec['sideband']),
                              polarization=unplain(spec['polarization']))


def build(meta, streams):
    cls = getattr(bt, meta['cls'])
    if meta['cls'] in ('Reshape', 'ReshapeAndTranspose', 'Transpose'):
        return cls(streams[0], *[tuple(a) for a in meta['args']])
    first = streams[0] if meta['cls'] in SHAPING else streams
    return cls(first, *[decode(a) for a in meta['args']], **meta['kwargs'])


def check_metadata(task, meta):
    """Shape, start time, framing and the three metadata arrays equal the reference's (by value)."""
    assert list(task.shape) == meta['shape']
    assert abs(task.start_time - u.Time(meta['start_time'])) < 1e-9
    assert task.samples_per_frame == meta['samples_per_frame']
    for attr in ('frequency', 'sideband', 'polarization'):
        want = unplain(meta[attr])
        got = getattr(task, attr, None)
        if want is None:
            assert got is None, attr
            continue
        got = np.asarray(got)
        assert got.shape == want.shape, (attr, got.shape, want.shape)
        assert np.array_equal(got, want.astype(got.dtype) if attr != 'polarization' else want), attr
