"""`ChunkedDeviceTask` (no GPU): the chunk loop of `_compute_frames` tiles a run of frames exactly and in
order, fetches what `_chunk_input` says and hands `_launch` the matching piece of the output;
`_input_span` names that fetch exactly when there is only one; the plan is made once and closed once."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import device_task
from baseband_tasks_amd.base import BaseTaskBase

T0 = bt.Time('2010-11-12T13:14:15')
N_OUT, HALO, SPF = 10, 2, 4


class Plan:
    closed = 0

    def close(self):
        self.closed += 1


class Halo(device_task.ChunkedDeviceTask, BaseTaskBase):
    """10 output samples in frames of 4, each needing its own input sample and the next two, as far as
    the stream goes."""
    chunk = 1

    def __init__(self, ih):
        self.plans, self.launches = [], []
        super().__init__(ih, shape=(N_OUT,), samples_per_frame=SPF)

    def _chunk_size(self):
        return self.chunk

    def _chunk_input(self, c0, c1):
        return c0, min(self.ih.shape[0], c1 + HALO) - c0

    def _make_plan(self):
        self.plans.append(Plan())
        return self.plans[-1]

    def _launch(self, x, start, count, out, c0, c1):
        self.plan_at_launch = self._plan
        self.launches.append((x, start, count, out.shape[0], c0, c1))
        out[...] = np.arange(c0, c1)


@pytest.fixture
def task(monkeypatch):
    ih = bt.HostStream(np.zeros((N_OUT + 1,), np.float32), T0, 1e4, samples_per_frame=SPF, pin=False)
    task = Halo(ih)
    task.fetches = []

    def fetch(stream, start, count):
        assert stream is ih
        task.fetches.append((start, count))
        return ('fetched', start, count)

    monkeypatch.setattr(device_task, 'fetch_device', fetch)
    return task


@pytest.mark.parametrize('chunk', [1, 3, 4, 100])
@pytest.mark.parametrize('first, last, a, b', [(0, 3, 0, 10), (1, 2, 4, 8)])
def test_the_chunks_tile_the_frames(task, chunk, first, last, a, b):
    task.chunk = chunk
    out = np.full(b - a, -1)
    task._compute_frames(first, last, out)
    bounds = [(c0, c1) for _, _, _, _, c0, c1 in task.launches]
    assert bounds[0][0] == a and bounds[-1][1] == b                               # exactly,
    assert all(p[1] == q[0] for p, q in zip(bounds, bounds[1:]))                  # in order, without gaps,
    assert all(0 < c1 - c0 <= chunk for c0, c1 in bounds)                         # within the chunk size
    assert len(bounds) == -(-(b - a) // chunk)
    assert task.fetches == [task._chunk_input(c0, c1) for c0, c1 in bounds]
    for (x, start, count, n_piece, c0, c1), fetched in zip(task.launches, task.fetches):
        assert x == ('fetched',) + fetched and (start, count) == fetched
        assert n_piece == c1 - c0
    assert np.array_equal(out, np.arange(a, b))                                   # every piece was out[c0 - a:c1 - a]
    if b == N_OUT:
        assert task.fetches[-1] == (bounds[-1][0], N_OUT + 1 - bounds[-1][0])     # (the halo, clipped at the end)
    if b - a <= chunk:
        assert len(task.fetches) == 1 and task._input_span(first, last) == (task.ih,) + task.fetches[0]
    else:
        assert len(task.fetches) > 1 and task._input_span(first, last) is None


def test_the_plan_is_made_once_and_closed_once(task):
    task.chunk = 3
    assert task._plan is None and not task.plans
    task._compute_frames(0, 3, np.zeros(10))
    task._compute_frames(1, 2, np.zeros(4))
    assert len(task.plans) == 1 and task._plan is task.plans[0] and task.plan_at_launch is task.plans[0]
    task._cache = object()
    task.close()
    assert task.plans[0].closed == 1 and task._plan is None and task._cache is None
    task.close()
    assert task.plans[0].closed == 1 and len(task.plans) == 1


def test_a_task_without_a_plan_closes(task, monkeypatch):
    monkeypatch.setattr(Halo, '_make_plan', device_task.ChunkedDeviceTask._make_plan)
    task._compute_frames(1, 2, np.zeros(4))
    assert task._plan is None and len(task.launches) == 4
    task.close()
    task.close()
