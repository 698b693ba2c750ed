"""Recover the ziggurat tables of NumPy's normal sampler (ki, wi, fi: 256 entries each) from the
installed NumPy and write them to baseband-tasks_amd/csrc/zig_tables.hpp (data only).

The tables are not part of NumPy's Python interface, so:
  1. wi[idx] is probed: a Philox bit generator whose ``buffer`` is written to hold the word
     ``idx | 1 << 9`` (rabs = 1, which every ki exceeds) makes `standard_normal` return exactly
     1 * wi[idx].
  2. The 2048 bytes of wi are searched for in NumPy's binaries (random/lib/libnpyrandom.a,
     random/_generator*.so); there fi is the 256 doubles directly before wi and ki the 256
     uint64 directly after it.  fi has to come from the binary: a few of its entries are one ulp
     off exp(-x_i^2 / 2) as evaluated today.
tests/test_noise_model.py checks the committed header against the running NumPy.

    python tools/make_zig_tables.py [--check]
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc', 'zig_tables.hpp')


def probe_word(word):
    """(the normal NumPy makes from `word` as the next word of the stream, buffer_pos afterwards)"""
    bg = np.random.Philox(0)
    st = bg.state
    # (the words behind it are uniforms of 0.5: a wedge or tail test they feed ends at once)
    st['buffer'] = np.array([word, 1 << 63, 1 << 63, 1 << 63], dtype=np.uint64)
    st['buffer_pos'] = 0
    bg.state = st
    x = np.random.Generator(bg).standard_normal()
    return x, bg.state['buffer_pos']


def probe_wi():
    return np.array([probe_word(idx | (1 << 9))[0] for idx in range(256)], dtype=np.float64)


def find_tables():
    wi = probe_wi()
    needle = wi.tobytes()
    d = os.path.dirname(np.random.__file__)
    for path in sorted(glob.glob(os.path.join(d, 'lib', 'libnpyrandom.a')) +
                       glob.glob(os.path.join(d, '_generator*.so'))):
        with open(path, 'rb') as f:
            blob = f.read()
        at = blob.find(needle)
        if at < 2048 or at + 4096 > len(blob):
            continue
        fi = np.frombuffer(blob, np.float64, 256, at - 2048)
        ki = np.frombuffer(blob, np.uint64, 256, at + 2048)
        # what the tables are: fi decreases from 1, ki are 52-bit thresholds
        if fi[0] == 1.0 and np.all(np.diff(fi) < 0) and fi[-1] > 0 and np.all(ki < (1 << 52)):
            return ki.copy(), wi, fi.copy(), os.path.relpath(path, d)
    raise RuntimeError('the ziggurat tables were not found in the NumPy binaries')


def render(ki, wi, fi):
    def block(name, bits):
        rows = [', '.join(f'0x{int(v):016x}ull' for v in bits[i:i + 4]) for i in range(0, 256, 4)]
        return f'#define {name} {{ \\\n    ' + ', \\\n    '.join(rows) + ' }\n'
    return ('// Ziggurat tables of NumPy\'s normal sampler (256 steps), as 64-bit patterns: ki as it is,\n'
            '// wi and fi the bits of the float64 values.  Data only; made by tools/make_zig_tables.py.\n'
            '#pragma once\n'
            + block('BBT_ZIG_KI', ki) + block('BBT_ZIG_WI', wi.view(np.uint64))
            + block('BBT_ZIG_FI', fi.view(np.uint64)))


def main():
    ki, wi, fi, where = find_tables()
    text = render(ki, wi, fi)
    if '--check' in sys.argv:
        with open(HEADER) as f:
            same = f.read() == text
        print('tables from', where, '-- header', 'matches' if same else 'DIFFERS')
        return 0 if same else 1
    with open(HEADER, 'w') as f:
        f.write(text)
    print('tables from', where, '->', os.path.relpath(HEADER, ROOT))
    return 0


if __name__ == '__main__':
    sys.exit(main())
