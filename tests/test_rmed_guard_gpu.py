"""`hip.RmedPlan.execute` between guard bands (tests/guard_bands.py): input and output each inside one
allocation between two bands of poison, 16-byte aligned and 4 bytes off, under NaN and +inf poison, the
stream made in one call and in chunks that are handed exactly the rows they need.  The shapes leave a
ragged tile (3 elements of 16) and the last chunk ends at the stream's end, so a load past the input
puts poison into a window -- which zeroes or moves outputs the twin has -- and a store past the output
shows in the bands."""
import numpy as np
import pytest

from baseband_tasks_amd import hip, search

import rmed_cases
from guard_bands import POISONS, SKEWS, Guarded, check_all
from rmed_cases import same_bits, set_tiling

pytestmark = pytest.mark.gpu

F32 = np.dtype(np.float32)
both_skews = pytest.mark.parametrize('skew', SKEWS, ids=['aligned16', 'off4'])
both_poisons = pytest.mark.parametrize('poison', list(POISONS.values()), ids=list(POISONS))
both_methods = pytest.mark.parametrize('select', [1, 2], ids=['radix', 'walk'])
#: (samples, width, scrunch, chunk): a scrunched stream with a dropped tail, and a plain one
SHAPES = pytest.mark.parametrize('n, w, s, chunk', [(37, 9, 2, 4), (23, 5, 1, 8)], ids=['w9-s2', 'w5-s1'])


def _words_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@both_poisons
@both_skews
@both_methods
@SHAPES
def test_guard_bands_whole(n, w, s, chunk, select, skew, poison, monkeypatch):
    set_tiling(monkeypatch, select)
    x = rmed_cases.noise()[:n, :3]
    rows = n // s
    plan = hip.RmedPlan(w, s, 3)
    for detrend, want in ((True, search.detrend_samples(x, w, s)), (False, search.running_median_samples(x, w, s))):
        gx, go = Guarded.load(x, poison, skew), Guarded(want.shape, F32, poison, skew)
        plan.execute(gx.array, 0, n, go.array, 0, rows * s, rows, detrend=detrend)
        got_x, got = check_all([gx, go], f'rmed whole detrend={detrend}')
        assert same_bits(got, want) and _words_equal(got_x, x) and np.isfinite(got).all() and got.any()
    plan.close()


@both_poisons
@both_skews
@both_methods
@SHAPES
def test_guard_bands_chunked(n, w, s, chunk, select, skew, poison, monkeypatch):
    """Every chunk gets a guarded input of exactly the rows `hip.rmed_info` says it needs: the first and
    the last begin and end at the stream's ends, where the windows are clipped and nothing lies beyond."""
    set_tiling(monkeypatch, select)
    x = rmed_cases.noise()[:n, :3]
    rows = n // s
    want = search.detrend_samples(x, w, s)
    plan = hip.RmedPlan(w, s, 3)
    for o0 in range(0, rows * s, chunk):
        o1 = min(rows * s, o0 + chunk)
        info = plan.info(rows, o0, o1 - o0)
        first, count = info['in_first'], info['in_count']
        assert 0 <= first and first + count <= rows * s
        piece = x[first:first + count]
        gx, go = Guarded.load(piece, poison, skew), Guarded((o1 - o0, 3), F32, poison, skew)
        plan.execute(gx.array, first, count, go.array, o0, o1 - o0, rows)
        got_x, got = check_all([gx, go], f'rmed chunk [{o0}, {o1})')
        assert same_bits(got, want[o0:o1]) and _words_equal(got_x, piece) and np.isfinite(got).all()
    assert o1 == rows * s and first + count == rows * s                 # the last chunk ends at the stream's end
    plan.close()
