"""The compact payloads of baseband_tasks_amd.hdf5 as the REAL h5py sees them, recorded once.

    python tests/golden/check_hdf5_compact.py write     # this package: writes compact_{c4,f2,bps8}.h5
    python tests/golden/check_hdf5_compact.py check     # an interpreter with h5py: writes compact_h5py.json

``write`` stores one small stream three ways with `HDF5StreamWriter` -- '<c4', '<f2' and 8-bit coded
words; ``check`` opens each file with h5py and records the payload's datatype, field names and
offsets, shape and the SHA-256 of the data it reads, with the versions of h5py and libhdf5.
tests/test_hdf5_coded_host.py holds the writer to the bytes of the three files and the record to
the values that were written, so it needs no h5py.  Recorded with h5py 3.3.0, libhdf5 1.10.6.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {'c4': dict(encoded_dtype='c4'), 'f2': dict(encoded_dtype='f2'), 'bps8': dict(bps=8)}


def samples(how):
    """(100, 2) samples, complex64 or (for 'f2') float32: sevenths, so that most round in half precision."""
    x = (((np.arange(400) * 37) % 101 - 50) / 7).astype(np.float32)
    return x[:200].reshape(100, 2) if how == 'f2' else x.view(np.complex64).reshape(100, 2)


def write():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from baseband_tasks_amd import hdf5
    for how, extra in CASES.items():
        x = samples(how)
        with hdf5.open(os.path.join(HERE, f'compact_{how}.h5'), 'w', shape=x.shape, dtype=x.dtype,
                       start_time='2020-01-01T00:00:00.5', sample_rate=16e6, frequency=np.array([1000e6, 1001e6]),
                       sideband=np.array([1, -1]), polarization=np.array(['X', 'Y']), **extra) as fw:
            fw.write(x)


def check():
    import h5py
    seen = dict(h5py=h5py.__version__, libhdf5=h5py.version.hdf5_version)
    for how in CASES:
        with h5py.File(os.path.join(HERE, f'compact_{how}.h5'), 'r') as fh:
            p = fh['payload']
            data = p[()]
            names = list(p.dtype.names or ())
            seen[how] = dict(dtype=str(p.dtype), names=names, shape=list(p.shape),
                             offsets=[int(p.dtype.fields[k][1]) for k in names],
                             sha256=hashlib.sha256(np.ascontiguousarray(data).tobytes()).hexdigest())
    with open(os.path.join(HERE, 'compact_h5py.json'), 'w') as f:
        json.dump(seen, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    {'write': write, 'check': check}[sys.argv[1]]()
