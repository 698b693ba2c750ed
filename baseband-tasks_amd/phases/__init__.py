"""Pulse phase predictors: the two-part `Phase`, tempo `Polyco` tables and the
`PolycoPhase` callable that `~baseband_tasks_amd.Fold`, `~baseband_tasks_amd.PulseStack`
and ``Integrate(phase=...)`` take (reference baseband_tasks/phases)."""
from .phase import Phase
from .predictor import Polyco
from .core import PolycoPhase

__all__ = ['Phase', 'Polyco', 'PolycoPhase']
