"""Mirror of the reference's ``simulator`` package: ``from simulator.solver import Simulator``."""
from .diagnostics import DIAG_FIELDS, DiagnosticsLog, DiagnosticsMixin, diagnostics_dict  # noqa: F401
